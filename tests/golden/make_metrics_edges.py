#!/usr/bin/env python3
"""Generate tests/golden/metrics_edges.npz: values of the reference's SinkhornDistance(eps, 100) and
MaximumMeanDiscrepancy (src/functions/metrics.py:107-273) on the compacted points of every frame of the sets `chunks`,
`sparse` and `small` of tests/metrics_edges_shapes.py, by IMPORTING the reference as make_metrics_frames.py does.

Runs only where the reference is checked out; the .npz it writes is committed and is what tests/test_metrics_edges.py
and tests/test_metrics_edges_gpu.py read.  Usage:  python tests/golden/make_metrics_edges.py

The inputs are not stored: the shapes module builds them from its seeds.  Per set and frame f (float64 arrays):
  <set>/ot32_<eps>[f]   SinkhornDistance(eps, 100)(x, y)[0] on the float32 points, eps in 0.01, 0.1, 1.0
  <set>/ot64_<eps>[f]   the same call on the points converted to float64
  <set>/mmd32[f], <set>/mmd64[f]   MaximumMeanDiscrepancy()(x, y) likewise
  <set>/count[f]        the present points (x, y), so that a change of the shapes module's seeds is noticed
|ot32 - ot64| is the reference's own float32-vs-float64 spread; a (set, eps) group's tolerance is 3 x the largest relative
spread among its frames, 1e-5 at the least (metrics_edges_shapes.cost_tolerance).  As generated:

  set     eps    3 x largest spread    tolerance
  chunks  0.01   4.0e-06               1.0e-05
  chunks  0.1    8.3e-07               1.0e-05
  chunks  1.0    3.5e-07               1.0e-05
  sparse  0.01   1.1e-03               1.1e-03
  sparse  0.1    4.9e-05               4.9e-05
  sparse  1.0    8.8e-06               1.0e-05
  small   0.01   8.4e-07               1.0e-05
  small   0.1    1.4e-06               1.0e-05
  small   1.0    2.8e-07               1.0e-05
The reference cannot run a frame with ONE point in y (sparse's last frame, 500 against 1): its 0-d v fails in M's
v.unsqueeze(-2).  That frame's ot32 / ot64 are NaN; the tests compare it with the float64 restatement and the closed form.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.join(REF, 'src'))
sys.path.insert(0, os.path.dirname(HERE))                                # tests/: the shapes module
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))               # the repository: piml_amd
sys.modules.setdefault('setproctitle', types.SimpleNamespace(setproctitle=lambda *_: None))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import functions.metrics as METRIC  # noqa: E402  (reference)

import metrics_edges_shapes as SH  # noqa: E402

torch.set_num_threads(8)
SETS = ('chunks', 'sparse', 'small')


def ot(sink, x, y):
    """the reference's value, NaN where it cannot run: with ONE point in y its nu and v are 0-d tensors after squeeze()
    and M's v.unsqueeze(-2) raises (one point in x passes, by broadcasting)"""
    try:
        return float(sink(x, y)[0])
    except IndexError:
        assert y.shape[0] == 1
        return np.nan


def main():
    out = {}
    mmd = METRIC.MaximumMeanDiscrepancy()
    print('set     eps    3 x largest spread    tolerance')
    for name in SETS:
        F = SH.n_frames(name)
        pts = [SH.compacted(name, f) for f in range(F)]
        out[f'{name}/count'] = np.array([[x.shape[0], y.shape[0]] for x, y in pts], np.int64)
        out[f'{name}/mmd32'] = np.array([float(mmd(x, y)) for x, y in pts], np.float64)
        out[f'{name}/mmd64'] = np.array([float(mmd(x.double(), y.double())) for x, y in pts], np.float64)
        for eps in SH.EPS:
            sink = METRIC.SinkhornDistance(eps=eps, max_iter=100, reduction=None)
            out[f'{name}/ot32_{eps}'] = np.array([ot(sink, x, y) for x, y in pts], np.float64)
            out[f'{name}/ot64_{eps}'] = np.array([ot(sink, x.double(), y.double()) for x, y in pts], np.float64)
            spread = np.abs(out[f'{name}/ot32_{eps}'] - out[f'{name}/ot64_{eps}']) / np.abs(out[f'{name}/ot64_{eps}'])
            print(f'{name:7s} {eps:<6} {3 * np.nanmax(spread):<21.1e} {SH.cost_tolerance(out, name, eps):.1e}')
    path = os.path.join(HERE, 'metrics_edges.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)')


if __name__ == '__main__':
    main()
