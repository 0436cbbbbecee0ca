#!/usr/bin/env python3
"""Generate tests/golden/scenario_gc.npz: the reference's Grand Central scenario (src/data/scenarios.py:313-401),
its utils.route (src/utils/utils.py:141-165) and its v2.2 clip writer (src/data/data.py:206-341), by IMPORTING the
reference as make_golden.py does.

Runs only where the reference is checked out; the .npz it writes is committed and is what tests/test_scenario.py and
tests/test_scenario_gpu.py read.  Usage:  python tests/golden/make_scenario_gc.py

Keys:
  wall (3994, 2), pillar (100, 2), entries (7, 100, 2)   GC()'s obstacles[0], obstacles[1] and entry tensors
  route/o, route/d (n, 2)   origin / destination pairs drawn as GC's get_od draws them (random.sample of two entries,
                            random.choice of a point, + torch.rand((1, 2)) * 0.8), seeded
  route/r (n, 2), route/iters (n)   the route point route() returns for the pair and the number of times it moved r
  clip/position, clip/destination (T, N, 2), clip/mask_p (T, N), clip/waypoints (D, N, 2), clip/obstacles (M, 2):
                            a small RawData grown with add_frame / add_pedestrians (agents entering late, leaving early,
                            one with a single waypoint)
  clip/traj (K, 4) = (agent, x, y, frame) rows of save_data's trajectories, clip/dest (L, 4) = (list index, x, y, frame)
  rows of its destinations, clip/dest_len: the length of each destination list
"""
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.join(REF, 'src'))
sys.modules.setdefault('setproctitle', types.SimpleNamespace(setproctitle=lambda *_: None))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import data.data as DATA  # noqa: E402  (reference)
import data.scenarios as SCEN  # noqa: E402  (reference)
import utils.utils as UTILS  # noqa: E402  (reference)

MAX_ITERS = 16          # the device's bound on route's loop (piml_amd.scenarios.Scenario.route_max_iters)


class _CountingTorch:
    """Stands in for `torch` inside utils.utils: counts torch.nonzero calls = moves of route()'s loop."""
    def __init__(self):
        self.calls = 0

    def nonzero(self, *a, **k):
        self.calls += 1
        return torch.nonzero(*a, **k)

    def __getattr__(self, name):
        return getattr(torch, name)


def entries_of(update):
    for c in update.__closure__:
        v = c.cell_contents
        if isinstance(v, list) and len(v) == 7:
            return v
    raise RuntimeError('GC entries not found')


def routes(entry, pillar, n, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    counter = _CountingTorch()
    UTILS.torch = counter
    try:
        O, D, R, I = [], [], [], []
        for _ in range(n):
            o, d = random.sample(entry, 2)
            o = o[random.choice(range(o.shape[0])), :].reshape(1, 2) + torch.rand((1, 2)) * 0.8
            d = d[random.choice(range(d.shape[0])), :].reshape(1, 2) + torch.rand((1, 2)) * 0.8
            before = counter.calls
            od = UTILS.route(torch.concat((o, d), dim=-2), pillar)
            O.append(o[0]); D.append(d[0]); R.append(od[1, 0]); I.append(counter.calls - before)
    finally:
        UTILS.torch = torch
    iters = np.array(I, np.int32)
    assert iters.max() < MAX_ITERS, iters.max()
    return torch.stack(O).numpy(), torch.stack(D).numpy(), torch.stack(R).numpy(), iters


def small_clip():
    """A reference RawData grown frame by frame: 3 agents at frame 0 (2 waypoints each), agent 3 enters at frame 2,
    agent 4 (one waypoint, the second NaN) at frame 3; agents leave when their flag passes the last waypoint."""
    nan = float('nan')
    wp = torch.tensor([[[2.0, 1.0], [5.0, 5.0], [1.0, 8.0]],
                       [[4.0, 0.5], [6.0, 9.0], [0.0, 9.5]]])                          # D=2, N=3
    pos0 = torch.tensor([[0.5, 0.5], [5.2, 4.1], [3.0, 7.0]])
    obstacles = torch.tensor([[10.0, 10.0], [10.5, 10.0], [11.0, 10.0]])
    raw = DATA.RawData(position=pos0.unsqueeze(0), velocity=torch.zeros(1, 3, 2), acceleration=torch.zeros(1, 3, 2),
                       destination=wp[:1].clone(), waypoints=wp.clone(), obstacles=obstacles, mask_p=torch.ones(1, 3),
                       mask_v=torch.ones(1, 3), mask_a=torch.ones(1, 3), meta_data={'time_unit': 0.08})
    raw.num_destinations = 2
    # frame -> agents whose flag advances in that frame's update
    arrive = {1: [1], 2: [0], 3: [1], 4: [0, 3], 5: [4], 6: [3]}
    for step in range(1, 8):
        frame = raw.get_frame(raw.num_steps - 1)
        frame = dict(frame)
        n = frame['num_pedestrians']
        frame['position'] = frame['position'] + torch.tensor([0.3, 0.2]) * step + 0.01 * torch.arange(n).unsqueeze(1)
        frame['velocity'] = torch.zeros(n, 2)
        frame['acceleration'] = torch.zeros(n, 2)
        for i in arrive.get(step, []):
            if i < n:
                frame['destination_flag'][i] += 1
        if step == 2:
            frame['num_pedestrians'] = n + 1
            frame['add_position'] = torch.tensor([[7.0, 1.0]])
            frame['add_velocity'] = torch.zeros(1, 2)
            frame['add_destination'] = torch.tensor([[[7.5, 3.0]], [[8.0, 6.0]]])
        if step == 3:
            frame['num_pedestrians'] = n + 1
            frame['add_position'] = torch.tensor([[2.0, 2.0]])
            frame['add_velocity'] = torch.zeros(1, 2)
            frame['add_destination'] = torch.tensor([[[3.0, 3.0]], [[nan, nan]]])
        raw.add_frame(frame)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'clip.npy')
        raw.save_data(path)
        meta, traj, dest, obs = np.load(path, allow_pickle=True)
    assert meta['version'] == 'v2.2'
    traj_rows = np.array([(a, x, y, f) for a, tr in enumerate(traj) for (x, y, f) in tr], np.float64)
    dest_rows = np.array([(a, x, y, f) for a, ds in enumerate(dest) for (x, y, f) in ds], np.float64)
    return {'clip/position': raw.position.numpy(), 'clip/destination': raw.destination.numpy(),
            'clip/mask_p': raw.mask_p.numpy(), 'clip/waypoints': raw.waypoints.numpy(), 'clip/obstacles': raw.obstacles.numpy(),
            'clip/traj': traj_rows, 'clip/dest': dest_rows, 'clip/dest_len': np.array([len(d) for d in dest], np.int32),
            'clip/traj_len': np.array([len(t) for t in traj], np.int32), 'clip/obstacles_list': np.array(obs, np.float64)}


def main():
    torch.manual_seed(0)
    random.seed(0)
    _, update, obstacles = SCEN.GC()
    entry = entries_of(update)
    out = {'wall': obstacles[0].numpy(), 'pillar': obstacles[1].numpy(), 'entries': torch.stack(entry).numpy()}
    o, d, r, it = routes(entry, obstacles[1], 2000, seed=1234)
    out.update({'route/o': o, 'route/d': d, 'route/r': r, 'route/iters': it})
    out.update(small_clip())
    path = os.path.join(HERE, 'scenario_gc.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: wall {out["wall"].shape}, routes {len(it)} (iterations {np.bincount(it).tolist()}), '
          f'clip {out["clip/position"].shape}')


if __name__ == '__main__':
    main()
