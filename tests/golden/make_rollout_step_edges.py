#!/usr/bin/env python3
"""Generate tests/golden/rollout_step_edges.npz: what the reference's BaseSimulator.get_multiple_rollouts
(src/models/simulators.py:556-657) makes of the cases REFERENCE of tests/rollout_step_shapes.py, on the CPU, by IMPORTING
the reference as make_metrics_edges.py does.

Runs only where the reference is checked out; the .npz it writes is committed and is what tests/test_rollout_step_ref.py
and tests/test_rollout_step_gpu.py read.  Usage:  python tests/golden/make_rollout_step_edges.py

The simulator is made with BaseSimulator.__new__ and given `args` (the feature geometry) and a stub in the network's place:
its k-th call returns a clone of a_table[..., t_start + k, :, :] (a clone: the reference writes into it, :634 and
src/data/data.py:483) and keeps a copy of the self_features it was handed.  The reference gets clones of the case: it
writes through its views into data.dest_idx[t_start] and data.self_features[t_start, :, 2:-3].

The inputs are not stored: the shapes module builds them from its seeds.  Per case (float32 arrays):
  <case>/position, velocity, acceleration (*c, T, N, 2), mask_p (*c, T, N)   the returned RawData
  <case>/self_features (T - t_start, *c, N, 2 H + 5)   what the stub was handed at frame t_start + k: destination - position,
                                                       the history, a and v0 of that frame
  <case>/count   int64: T, N, D, H, C (0: no channel axis), t_start -- so that a change of the shapes module is noticed
The reference cannot run `shared_wp` (slices with (D, N, 2) waypoints: the gather of :616 raises on the index's extra
axis), which is checked here, and no case has N = 1 (its squeeze() calls of :616, :647-649 would drop the agent axis)."""
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

import models.simulators as SIM  # noqa: E402  (reference)

import rollout_step_shapes as SH  # noqa: E402

torch.set_num_threads(1)


class Stub:
    """stands where the network does: the table's rows in order, and a record of what it was asked with"""

    def __init__(self, a_table, t_start):
        self.a_table, self.k, self.seen = a_table, t_start, []

    def __call__(self, ped_features, obs_features, self_features):
        self.seen.append(self_features.clone())
        out = self.a_table[..., self.k, :, :].clone()
        self.k += 1
        return (out,)


def simulator(stub):
    sim = SIM.BaseSimulator.__new__(SIM.BaseSimulator)
    sim.args = types.SimpleNamespace(device='cpu', topk_ped=SH.KP, topk_obs=SH.KO, sight_angle_ped=90, sight_angle_obs=90,
                                     dist_threshold_ped=4, dist_threshold_obs=4)
    sim.model = stub
    sim.finetune_flag = False
    return sim


def run(name):
    data, a_table, t_start = SH.case(name)
    stub = Stub(a_table, t_start)
    with torch.no_grad():
        out = simulator(stub).get_multiple_rollouts(data, t_start=t_start, load_model=False)
    return out, torch.stack(stub.seen), data, t_start


def main():
    res = {}
    for name in SH.REFERENCE:
        out, seen, data, t_start = run(name)
        for k in ('position', 'velocity', 'acceleration', 'mask_p'):
            res[f'{name}/{k}'] = getattr(out, k).numpy().astype(np.float32)
        res[f'{name}/self_features'] = seen.numpy().astype(np.float32)
        spec = SH.SPECS['multi_wp' if name == 'late_start' else name]
        res[f'{name}/count'] = np.array([spec['T'], spec['N'], spec['D'], spec['H'], spec['C'] or 0, t_start], np.int64)
        print(f'{name:11s} {tuple(out.position.shape)} frames seen {seen.shape[0]}  {SH.events(name)}')
    try:
        run('shared_wp')
    except RuntimeError as ex:
        print('shared_wp: the reference raises,', str(ex).splitlines()[0])
    else:
        raise SystemExit('shared_wp: the reference ran (D, N, 2) waypoints with a channel axis; record it')
    path = os.path.join(HERE, 'rollout_step_edges.npz')
    np.savez_compressed(path, **res)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)')


if __name__ == '__main__':
    main()
