#!/usr/bin/env python3
"""Generate tests/golden/scenario_synth.npz: the reference's synthetic scenes (src/data/scenarios.py:9-311: crosswalk,
four_directional_square, basic_unit1..3), by IMPORTING the reference as make_scenario_gc.py does.

Runs only where the reference is checked out (PIML_REFERENCE=<its checkout>); the .npz it writes is committed and is what tests/test_scenario_synth.py and
tests/test_scenario_synth_gpu.py read.  Usage:  PIML_REFERENCE=<checkout> python tests/golden/make_scenario_synth.py

A scene's `generate` is a closure of its update function: it is reached through `update`, called on a one-agent fake frame
while torch.poisson returns a fixed count (the agents it generates are frame['add_*']).  Keys, per scene S:
  S/frame0/position, velocity (N, 2), waypoints (D, N, 2), desired_speed (N), obstacles (M, 2)
                     the frame-0 SocialForceData the factory returns under torch.manual_seed(0)
  S/gen/<column>     20000 agents of one `update` call (torch.manual_seed(1)); for basic_unit3 g1/ and g2/ separately
                     (counts (n, 0) and (0, n)); the basic units with uniform_desired_speed=False (their speed law's draws).
                     Columns: x, y (position), dx, dy (waypoint 0), dx1, dy1 (the crosswalk's waypoint 1), v0 (desired
                     speed); the crosswalk's x as x_side (its sign) and abs_x.  A column with at most two values (a constant
                     or a coin) is float32 in agent order, exact; any other is float16, SORTED: the tests use only its
                     marginal distribution (range, mean, two-sample KS), which a 2^-11 relative rounding moves by < 1e-3 in
                     the KS statistic (the 1e-3 critical value at n = m = 20000 is 0.0195), and it keeps the file small.
  four_directional_square/unshuffled/position, waypoints: frame 0 with torch.randperm patched to arange
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('PIML_REFERENCE', '')     # a checkout of the reference (tsinghua-fib-lab/PIML)
if not os.path.isdir(os.path.join(REF, 'src')):
    sys.exit('set PIML_REFERENCE to a checkout of the reference')
sys.path.insert(0, os.path.join(REF, 'src'))
sys.modules.setdefault('setproctitle', types.SimpleNamespace(setproctitle=lambda *_: None))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import data.scenarios as SCEN  # noqa: E402  (reference)

N_GEN = 20000


def frame0(out, key, data):
    out[f'{key}/frame0/position'] = data.position[0].numpy()
    out[f'{key}/frame0/velocity'] = data.velocity[0].numpy()
    out[f'{key}/frame0/waypoints'] = data.waypoints.numpy()
    out[f'{key}/frame0/desired_speed'] = data.desired_speed.numpy()
    out[f'{key}/frame0/obstacles'] = np.asarray(data.obstacles, np.float32).reshape(-1, 2)


def generated(update, counts):
    """the agents one update call generates while torch.poisson returns `counts` in turn"""
    it = iter(counts)
    poisson = torch.poisson
    torch.poisson = lambda x: torch.tensor(float(next(it)))
    try:
        frame = {'position': torch.zeros(1, 2), 'destination': torch.full((1, 2), 100.0),
                 'destination_flag': torch.zeros(1, dtype=torch.int), 'mask_p': torch.ones(1), 'num_pedestrians': 1}
        torch.manual_seed(1)
        frame = update(frame)
    finally:
        torch.poisson = poisson
    return {'position': frame['add_position'].numpy(), 'waypoints': frame['add_destination'].numpy(),
            'desired_speed': frame['add_desired_speed'].numpy()}


def put(out, prefix, gen):
    p, w, v0 = (np.asarray(gen[k], np.float32) for k in ('position', 'waypoints', 'desired_speed'))
    cols = {'x': p[:, 0], 'y': p[:, 1], 'dx': w[0, :, 0], 'dy': w[0, :, 1], 'v0': v0}
    if w.shape[0] > 1:
        cols.update(dx1=w[1, :, 0], dy1=w[1, :, 1])
    if len(np.unique(cols['x'])) > 2 and (cols['x'] < 0).any():          # the crosswalk: a coin side times a distance
        x = cols.pop('x')
        cols.update(x_side=np.sign(x).astype(np.float32), abs_x=np.abs(x))
    for k, c in cols.items():
        out[f'{prefix}/{k}'] = c if len(np.unique(c)) <= 2 else np.sort(c).astype(np.float16)


def main():
    out = {}
    torch.manual_seed(0)
    data, update = SCEN.crosswalk()
    frame0(out, 'crosswalk', data)
    put(out, 'crosswalk/gen', generated(update, [N_GEN]))

    torch.manual_seed(0)
    data, _ = SCEN.four_directional_square()
    frame0(out, 'four_directional_square', data)
    randperm = torch.randperm
    torch.randperm = lambda n, *a, **k: torch.arange(n)
    try:
        data, _ = SCEN.four_directional_square()
    finally:
        torch.randperm = randperm
    out['four_directional_square/unshuffled/position'] = data.position[0].numpy()
    out['four_directional_square/unshuffled/waypoints'] = data.waypoints.numpy()

    for key, fn, counts in (('basic_unit1', SCEN.basic_unit1, [[N_GEN]]), ('basic_unit2', SCEN.basic_unit2, [[N_GEN]]),
                            ('basic_unit3', SCEN.basic_unit3, [[N_GEN, 0], [0, N_GEN]])):
        torch.manual_seed(0)
        data, update = fn()
        frame0(out, key, data)
        _, update = fn(uniform_desired_speed=False)          # (the speed law's normal draws too)
        for g, c in enumerate(counts):
            put(out, f'{key}/gen' + (f'/g{g + 1}' if len(counts) > 1 else ''), generated(update, c))
    path = os.path.join(HERE, 'scenario_synth.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
