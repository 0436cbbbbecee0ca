"""What can be checked of the inference-rollout step cases (tests/rollout_step_shapes.py) without a GPU: the numpy restatement
of one frame (tests/rollout_step_ref.py) against the reference's own run recorded in tests/golden/rollout_step_edges.npz, the
conditions the cases were built to meet, and the eager torch frame (BaseSimulator._rollout_step) on the CPU against the
restatement.  Everything is compared bit for bit, a NaN equal to any NaN."""
import types

import numpy as np
import pytest
import torch

from conftest import golden

import rollout_step_ref as R
import rollout_step_shapes as SH


@pytest.fixture(scope='module')
def recorded():
    return golden('rollout_step_edges')


@pytest.mark.parametrize('name', SH.REFERENCE)
def test_restatement_equals_recorded_reference(recorded, name):
    """position, velocity, acceleration, mask_p of the result, and the self_features the network was handed at every frame:
    destination - position (the destination of the frame), the history, a, v0"""
    data, _, t_start = SH.case(name)
    spec = SH.SPECS['multi_wp' if name == 'late_start' else name]
    assert recorded[f'{name}/count'].tolist() == [spec['T'], spec['N'], spec['D'], spec['H'], spec['C'] or 0, t_start]
    final, records = SH.restated(name)
    for k, want in (('p_res', 'position'), ('v_res', 'velocity'), ('a_res', 'acceleration'), ('mask', 'mask_p')):
        assert R.differs(getattr(final, k), recorded[f'{name}/{want}']) == 0, (name, want)
    seen = recorded[f'{name}/self_features']
    assert seen.shape[0] == spec['T'] - t_start == len(records)
    assert R.differs(data.self_features[..., t_start, :, :].numpy(), seen[0]) == 0
    for k in range(1, seen.shape[0]):                    # the row the frame before wrote
        assert R.differs(records[k - 1].selff, seen[k]) == 0, (name, t_start + k)


@pytest.mark.parametrize('name', SH.ALL)
def test_cases_meet_their_conditions(name):
    ev = SH.events(name)
    # a last-bit difference between torch.norm and the kernel's sqrt(fma(y, y, x * x)) cannot flip a switch
    assert ev['margin'] > SH.MARGIN, (name, ev)
    if name in SH.REFERENCE:
        assert SH.SPECS['multi_wp' if name == 'late_start' else name]['N'] > 1
        for k, least in SH.MIN_EVENTS.items():
            assert ev[k] >= least, (name, k, ev)


@pytest.mark.parametrize('name', ('multi_wp', 'hist3', 'hist2', 'slices', 'shared_wp'))
def test_hand_placed_agents_do_what_they_were_placed_for(name):
    data, _, t_start = SH.case(name)
    assert t_start == 0
    T = data.num_frames
    final, rec = SH.restated(name)
    r = SH.ROLES
    first = rec[0]
    assert not first.events.near[..., r['exact_x']].any() and (first.dest_idx[..., r['exact_x']] == 0).all()   # strict <
    assert first.events.near[..., r['below_x']].all() and (first.dest_idx[..., r['below_x']] == 1).all()
    assert not first.events.near[..., r['exact_y']].any() and (first.dest_idx[..., r['exact_y']] == 0).all()
    i = r['arrive_enter']
    both = np.stack([x.events.gone[..., i] & x.events.enter[..., i] for x in rec], -1)               # (*c, frames)
    assert (both.sum(-1) == 1).all()
    for c, row in enumerate(both.reshape(-1, T)):
        k = int(np.argmax(row))
        p = final.p_res.reshape(-1, T, *final.p_res.shape[-2:])[c, k + 1, i]
        assert not np.isnan(p).any(), 'the injection wins: no NaN'
    i = r['never']
    assert np.isnan(final.p_res[..., i, :]).all() and (final.mask[..., i] == 0).all()
    assert np.isnan(rec[0].hist[..., i, :]).all(), 'its NaN velocity enters the history'
    assert np.isnan(final.v_res[..., 0, i, :]).all() and (final.v_res[..., 1, i, :] == 0).all(), 'and is 0 in the state (data.py:484)'
    assert not np.isnan(final.v_res[..., 1:, i, :]).any()
    assert (final.a_res[..., 3, i, :] == 0).all(), 'as a NaN of the network (data.py:483)'
    for i, frame in ((r['enter_1'], 1), (r['enter_last'], T - 1)):
        assert (final.mask[..., :frame, i] == 0).all() and (final.mask[..., frame, i] == 1).all()
        assert rec[frame - 1].events.enter[..., i].all()
    assert (data.dest_num[[r['one_wp'], r['arrive_enter']]] == 1).all()
    assert set(data.dest_num.tolist()) == set(range(1, data.waypoints.shape[-3] + 1))                # dest_num drawn from 1..D


def test_shared_waypoints_are_the_per_slice_run_on_broadcast_waypoints():
    """what `shared_wp` is compared with on the GPU: the reference cannot run it, the restatement's shared gather is the
    per-slice gather (the reference's, bit for bit above) on the same waypoints repeated for every slice"""
    data, a_table, t_start = SH.case('shared_wp')
    C = data.position.shape[0]
    assert data.waypoints.dim() == 3
    wide = SH.clone(data)
    wide.waypoints = data.waypoints.unsqueeze(0).repeat(C, 1, 1, 1)
    final, rec = SH.restated('shared_wp')
    final_w, rec_w = R.run(R.series(wide), a_table.numpy(), t_start)
    for k in ('p_res', 'v_res', 'a_res', 'mask', 'dest', 'dest_idx', 'hist'):
        assert R.differs(getattr(final, k), getattr(final_w, k)) == 0, k
    for a, b in zip(rec, rec_w):
        assert R.differs(a.selff, b.selff) == 0
    other, _ = SH.restated('slices')                     # and it is not the run on the slices' own waypoints
    assert R.differs(final.dest[1:], other.dest[1:]) > 0 and R.differs(final.dest[0], other.dest[0]) == 0


class TableModel:
    """stands where the network does: a_table's rows in order"""

    def __init__(self, a_table, t_start):
        self.a_table, self.k = a_table, t_start

    def __call__(self, ped_features, obs_features, self_features):
        out = self.a_table[..., self.k, :, :].clone()
        self.k += 1
        return (out,)


def make_simulator(model, device='cpu'):
    from piml_amd.models.simulators import BaseSimulator
    sim = BaseSimulator.__new__(BaseSimulator)
    sim.args = types.SimpleNamespace(device=device, topk_ped=SH.KP, topk_obs=SH.KO, sight_angle_ped=90, sight_angle_obs=90,
                                     dist_threshold_ped=4, dist_threshold_obs=4, num_history_velocity=1)
    sim.model = model
    sim.finetune_flag = False
    return sim


@pytest.mark.parametrize('name', [n for n in SH.ALL if n != 'shared_wp'])
def test_eager_torch_frame_equals_restatement_on_the_cpu(name, monkeypatch):
    """BaseSimulator._rollout_step (what test_simulator_gpu.py calls `eager`) frame by frame.  Only the feature kernel behind
    Pedestrians.get_relative_features is replaced (it has no CPU path): by zero neighbour features and destination - position,
    NaN -> 0.  The NaN -> 0 that get_relative_features writes into the frame's v and a stays in the path.  Shared waypoints
    with a channel axis are the fused kernel's only: the eager frame's gather raises on them as the reference's does."""
    from piml_amd import ops

    def features(position, velocity, acceleration, destination, obstacles, *geometry, heading=None):
        lead = position.shape[:-1]
        return (torch.zeros(*lead, SH.KP, 6), torch.zeros(*lead, SH.KO, 6), torch.nan_to_num(destination - position, nan=0.0))
    monkeypatch.setattr(ops, 'relative_features', features)
    data, a_table, t_start = SH.case(name)
    sim = make_simulator(TableModel(a_table, t_start))
    final, rec = SH.restated(name)
    with torch.no_grad():
        st = sim._rollout_state(data, t_start)
        for t in range(t_start, data.num_frames):
            sim._rollout_step(data, st)
            assert int(st.t) == t + 1
            assert R.state_differences(st, rec[t - t_start], final, t, head=True) == {}, (name, t)
    for k, want in (('p_res', final.p_res), ('v_res', final.v_res), ('a_res', final.a_res), ('mask_new', final.mask)):
        assert R.differs(getattr(st, k).numpy(), want) == 0, k
