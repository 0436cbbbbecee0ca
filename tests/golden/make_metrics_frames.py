#!/usr/bin/env python3
"""Generate tests/golden/metrics_frames.npz: PER-FRAME values of the reference's Sinkhorn OT and MMD
(src/functions/metrics.py:94-273), by IMPORTING the reference as make_golden.py does.

Runs only where the reference is checked out; the .npz it writes is committed and is what
tests/test_metrics_hip.py and tests/test_metrics_hip_gpu.py read.  Usage:  python tests/golden/make_metrics_frames.py

Sets (each: p, q (T, N, 2) float32, mask (T, N); absent slots hold NaN):
  gc     a perturbed 12-frame window of the 219-agent GC clip time2224-2284 (up to 51 present agents per frame)
  ucy    a perturbed 12-frame window of the 144-agent UCY clip time0-54
  syn512 / syn1024   seeded synthetic frames of 512 / 1024 slots, ~5 % of them absent
  edge   frames with 0, 1 and 2 present agents and one whose points all coincide (MMD NaN)
Per set and frame f:  <set>/ot[f] = SinkhornDistance(0.1, 100)(p[f][mask], q[f][mask]) (NaN where fewer than 2 agents),
<set>/mmd32[f] = MaximumMeanDiscrepancy()(...) on float32, <set>/mmd64[f] the same on float64 inputs (the reference's own
float32-vs-float64 spread is |mmd32 - mmd64|).
Unequal clouds (n != m): uneq{k}/x, uneq{k}/y and wasserstein_distance_2d's dist, P, C, mmd_loss on float32 / float64.
A batch of three (30 vs 40 points) through wasserstein_distance_2d: batch/x, batch/y, batch/dist.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.join(REF, 'src'))
sys.modules.setdefault('setproctitle', types.SimpleNamespace(setproctitle=lambda *_: None))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import data.data as DATA  # noqa: E402  (reference)
import functions.metrics as METRIC  # noqa: E402  (reference)

torch.set_num_threads(8)
GC = os.path.join(REF, 'data/GC_Dataset/GC_Dataset_ped1-12685_time2224-2284_interp9_xrange5-25_yrange15-35.npy')
UCY = os.path.join(REF, 'data/UCY_dataset/UCY_Dataset_time0-54_timeunit0.08.npy')


def clip_window(path, t0, frames, seed):
    raw = DATA.RawData()
    raw.load_trajectory_data(path)
    q = raw.position[t0:t0 + frames].clone().float()
    mask = (raw.mask_p[t0:t0 + frames] == 1).float()
    g = torch.Generator().manual_seed(seed)
    p = q + 0.3 * torch.randn(q.shape, generator=g)
    return p, q, mask


def synthetic(frames, N, seed):
    g = torch.Generator().manual_seed(seed)
    q = 20 * torch.rand(frames, N, 2, generator=g)
    p = q + 0.3 * torch.randn(q.shape, generator=g)
    mask = (torch.rand(frames, N, generator=g) >= 0.05).float()
    return p, q, mask


def edge():
    q = torch.tensor([[0.5, 1.0], [2.0, 0.5], [1.0, 3.0], [4.0, 4.5]]).repeat(4, 1, 1)
    p = q + torch.tensor([[0.2, -0.1], [0.3, 0.4], [-0.5, 0.1], [0.1, 0.2]])
    mask = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1], [1, 1, 1, 1]], dtype=torch.float32)
    p[3], q[3] = 7.0, 7.0                                                 # every point of frame 3 coincides
    return p, q, mask


def per_frame(p, q, mask):
    ot, mmd32, mmd64 = [], [], []
    sink = METRIC.SinkhornDistance(eps=0.1, max_iter=100, reduction=None)
    mmd = METRIC.MaximumMeanDiscrepancy()
    for f in range(p.shape[0]):
        sel = mask[f] == 1
        x, y = p[f][sel], q[f][sel]
        if int(sel.sum()) < 2:
            ot.append(np.nan), mmd32.append(np.nan), mmd64.append(np.nan)
            continue
        ot.append(float(sink(x, y)[0]))
        mmd32.append(float(mmd(x, y)))
        mmd64.append(float(mmd(x.double(), y.double())))
    return np.array(ot, np.float64), np.array(mmd32, np.float64), np.array(mmd64, np.float64)


def main():
    out = {}
    sets = dict(gc=clip_window(GC, 700, 12, 11), ucy=clip_window(UCY, 480, 12, 12), syn512=synthetic(3, 512, 13),
                syn1024=synthetic(2, 1024, 14), edge=edge())
    for name, (p, q, mask) in sets.items():
        ot, mmd32, mmd64 = per_frame(p, q, mask)
        absent = (mask == 0).unsqueeze(-1)
        out.update({f'{name}/p': torch.where(absent, float('nan'), p).numpy(),
                    f'{name}/q': torch.where(absent, float('nan'), q).numpy(),
                    f'{name}/mask': mask.numpy(), f'{name}/ot': ot, f'{name}/mmd32': mmd32, f'{name}/mmd64': mmd64})
        print(name, tuple(p.shape), 'agents per frame', mask.sum(-1).int().tolist())
    g = torch.Generator().manual_seed(15)
    for k, (n, m) in enumerate(((37, 53), (100, 70))):
        x = 10 * torch.rand(n, 2, generator=g)
        y = 10 * torch.rand(m, 2, generator=g) + 0.5
        dist, P, C = METRIC.wasserstein_distance_2d(x, y)
        out.update({f'uneq{k}/x': x.numpy(), f'uneq{k}/y': y.numpy(), f'uneq{k}/dist': np.float64(dist),
                    f'uneq{k}/P': P.numpy(), f'uneq{k}/C': C.numpy(),
                    f'uneq{k}/mmd32': np.float64(METRIC.mmd_loss(x, y)),
                    f'uneq{k}/mmd64': np.float64(METRIC.mmd_loss(x.double(), y.double()))})
    # 3-D (batched) input: the reference stops the whole batch on the MEAN err of its frames (metrics.py:168)
    x = 10 * torch.rand(3, 30, 2, generator=g)
    y = torch.cat((x[:1] + 0.1 * torch.randn(1, 30, 2, generator=g), 10 * torch.rand(2, 30, 2, generator=g)))
    y = torch.cat((y, 10 * torch.rand(3, 10, 2, generator=g)), dim=1)
    out.update({'batch/x': x.numpy(), 'batch/y': y.numpy(), 'batch/dist': METRIC.wasserstein_distance_2d(x, y)[0].numpy()})
    path = os.path.join(HERE, 'metrics_frames.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)')


if __name__ == '__main__':
    main()
