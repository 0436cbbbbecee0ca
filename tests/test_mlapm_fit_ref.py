"""CPU: the float64 yardstick of the calibration kernels (tests/mlapm_fit_ref.py) against the values the reference's own
autograd recorded (tests/golden/mlapm_fit.npz, mlapm_rollout_fit.npz), and its scene builders and pack editors against
what they claim to build."""
import os

import numpy as np
import pytest
import torch

import mlapm_fit_ref as R
from conftest import REPO, golden

GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
LAW = {'tau': 0.7, 'A': 5.0, 'B': -2.0, 'C': 0.3, 'D': -0.2, 'theta': 40.0}
TRUTH = {'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}


@pytest.fixture(scope='module')
def gc_clip():
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(REPO, 'tests', 'golden', 'data', GC_CLIP))
    return raw, R.desired_speed64(raw)


def agree(tag, loss, grad, want, gw, scale, rel=1e-9):
    assert abs(loss - want) <= rel * want, (tag, loss, want)
    for q, name in enumerate(R.NAMES):
        if scale[q] == 0:
            assert grad[q] == 0.0, (tag, name, grad[q])
        else:
            assert abs(grad[q] - gw[q]) <= rel * scale[q], (tag, name, grad[q], gw[q], scale[q])


@pytest.mark.parametrize('version', ['raw', 'GC'])
def test_one_step_yardstick_reproduces_the_reference_autograd(gc_clip, version):
    from piml_amd.calibrate import pack_clip
    raw, v0 = gc_clip
    g = golden('mlapm_fit')
    pack = pack_clip(raw, frames=[int(f) for f in g['frames']], device='cpu')
    for k in range(2):
        tag = f'{version}_{k}'
        assert pack.num_focal == int(g[f'count_{tag}'])
        params = dict(zip(R.NAMES, g[f'params_{tag}']))
        loss, grad, scale = R.fit_reference(pack, params, version, float(g['dt']), float(g['radius']), desired_speed=v0,
                                            scale=True)
        assert np.allclose(scale, g[f'grad_scale_{tag}'], rtol=1e-9, atol=0), (tag, scale, g[f'grad_scale_{tag}'])
        agree(tag, loss, grad, float(g[f'loss_{tag}']), g[f'grad_{tag}'], g[f'grad_scale_{tag}'])


@pytest.mark.parametrize('version', ['raw', 'GC'])
def test_rollout_yardstick_reproduces_the_reference_autograd(gc_clip, version):
    raw, v0 = gc_clip
    g = golden('mlapm_rollout_fit')
    H, starts = int(g['horizon']), [int(x) for x in g['starts']]
    clip = R.clip_arrays(raw, v0)
    for k in range(2):
        for q, decay in enumerate(g['decays']):
            tag = f'{version}_{k}_{q}'
            params = dict(zip(R.NAMES, g[f'params_{tag}']))
            loss, grad, sse, cnt, scale = R.rollout_reference(clip, starts, H, params, version, float(g['dt']),
                                                              float(g['radius']), float(decay), scale=True)
            assert np.array_equal(cnt, g[f'step_count_{tag}']) and int(cnt.sum()) == int(g[f'count_{tag}'])
            assert np.allclose(sse, g[f'sse_{tag}'], rtol=1e-9, atol=0), (tag, sse, g[f'sse_{tag}'])
            assert np.allclose(scale, g[f'grad_scale_{tag}'], rtol=1e-9, atol=0), (tag, scale)
            agree(tag, loss, grad, float(g[f'loss_{tag}']), g[f'grad_{tag}'], g[f'grad_scale_{tag}'])


def test_check_against_holds_its_bars():
    gw = np.array([1.0, -2.0, 1e-6, 0.0, 0.0, 0.0])
    R.check_against(3.0, gw.copy(), None, 3.0, gw, None, None, version='raw')
    with pytest.raises(AssertionError):
        R.check_against(3.0 * (1 + 2e-5), gw.copy(), None, 3.0, gw, None, None)
    with pytest.raises(AssertionError):                                   # the largest gradient 3e-5 off
        R.check_against(3.0, gw * np.array([1, 1 + 3e-5, 1, 1, 1, 1]), None, 3.0, gw, None, None)
    with pytest.raises(AssertionError):                                   # a small one more than 1e-5 of 1e-3 of the largest off
        R.check_against(3.0, gw + np.array([0, 0, 5e-8, 0, 0, 0]), None, 3.0, gw, None, None)
    with pytest.raises(AssertionError):                                   # a constant raw does not use, not exactly 0
        R.check_against(3.0, gw + np.array([0, 0, 0, 1e-12, 0, 0]), None, 3.0, gw, None, None, version='raw')
    sse, cnt = np.array([1.0, 2.0]), np.array([3.0, 4.0])
    R.check_against(3.0, gw.copy(), np.array([1.0, 2.0, 3.0, 4.0]), 3.0, gw, sse, cnt)
    with pytest.raises(AssertionError):
        R.check_against(3.0, gw.copy(), np.array([1.0, 2.0, 3.0, 5.0]), 3.0, gw, sse, cnt)
    with pytest.raises(AssertionError):
        R.check_against(3.0, gw.copy(), np.array([1.0, 2.001, 3.0, 4.0]), 3.0, gw, sse, cnt)


def test_flow_clip_is_the_law_it_was_simulated_at():
    """Every agent present, finite and moving ahead; the yardstick's one-step and rollout losses at the truth law are the
    float32 storage's rounding, and at another law they are not."""
    from piml_amd.calibrate import pack_clip
    for version in ('raw', 'GC', 'UCY'):
        # UCY: closer than its collision distance 2 radius = 0.6 m here and there, or B and C never enter
        spacing = 0.6 if version == 'UCY' else 1.5
        raw = R.flow_clip(30, 12, TRUTH, version, spacing=spacing, seed=3)
        assert tuple(raw.position.shape) == (12, 30, 2) and raw.position.dtype == torch.float32
        assert torch.isfinite(raw.position).all() and torch.isfinite(raw.velocity).all()
        d = torch.cdist(raw.position[0], raw.position[0]) + 10 * torch.eye(30)
        # lattice neighbours: 1 - 2 jitter along the axis at the least, 1 + 2 jitter and 2 jitter across at the most
        assert spacing * 0.7 <= float(d.min()) and float(d.min(1).values.max()) <= spacing * (1.3 ** 2 + 0.3 ** 2) ** 0.5
        head = raw.position[-1] - raw.position[0]
        ang = torch.rad2deg(torch.atan2(head[:, 1], head[:, 0]))
        # (UCY pushes every pair in view with the full A whatever the distance: its crowd fans out)
        assert version == 'UCY' or (float((ang - 27).abs().max()) < 40 and float(head.norm(dim=-1).min()) > 0.3)
        pack = pack_clip(raw, desired_speed=1.3, device='cpu')
        assert pack.num_focal == 11 * 30
        at, _ = R.fit_reference(pack, TRUTH, version, 0.08)
        off, g = R.fit_reference(pack, LAW, version, 0.08)
        assert at < 1e-12 and off > 1e-4, (version, at, off)
        used = [q for q in range(6) if q not in R.UNUSED[version]]
        assert all(g[q] != 0 for q in used) and all(g[q] == 0 for q in R.UNUSED[version]), (version, g)
        at, _, _, cnt = R.rollout_reference(raw, [0, 3], 8, TRUTH, version, 0.08, desired_speed=1.3)
        off, _, _, _ = R.rollout_reference(raw, [0, 3], 8, LAW, version, 0.08, desired_speed=1.3)
        assert at < 1e-11 and off > 1e-5 and np.array_equal(cnt, np.full(8, 60.0)), (version, at, off, cnt)


def test_presence_patterns_give_the_flags_they_claim():
    from piml_amd.calibrate import pack_windows
    H, t0, T = 8, 2, 14
    base = R.flow_clip(9, T, TRUTH, 'GC', seed=1)
    pats = R.presence_patterns(t0, H, T)
    names = sorted(pats)
    assert names == ['enter', 'first_only', 'gap', 'last_only', 'leave', 'one_mid']
    raw = R.with_presence(base, {a + 1: pats[name] for a, name in enumerate(names)})       # agents 0, 7, 8 stay whole
    assert torch.equal(torch.isnan(raw.position).any(-1), torch.isnan(raw.velocity).any(-1))
    assert torch.isfinite(base.position).all()                                              # the edit is a copy
    pack = pack_windows(raw, H, frames=f'{t0}:{t0 + H + 1}', desired_speed=1.3, device='cpu')
    assert pack.num_windows == 1 and pack.slot_count == [9] and pack.start == [t0]
    flags = pack.flags.reshape(H + 1, 9).t().tolist()                                       # (slot, k)
    whole = [3] + [5] * H
    assert flags[0] == whole and flags[7] == whole and flags[8] == whole
    # by hand, k = 0 .. 8: bit 0 present, bit 1 injected, bit 2 carried
    assert flags[1 + names.index('leave')] == [3, 5, 5, 0, 0, 0, 0, 0, 0]
    assert flags[1 + names.index('enter')] == [0, 0, 0, 3, 5, 5, 5, 5, 5]
    assert flags[1 + names.index('gap')] == [3, 5, 5, 0, 0, 3, 5, 5, 5]
    assert flags[1 + names.index('first_only')] == [3, 0, 0, 0, 0, 0, 0, 0, 0]
    assert flags[1 + names.index('last_only')] == [0, 0, 0, 0, 0, 0, 0, 0, 3]
    assert flags[1 + names.index('one_mid')] == [0, 0, 0, 3, 0, 0, 0, 0, 0]
    for a, name in enumerate(names):
        assert flags[1 + a] == R.expected_flags(name, H), name
    # k = 1 .. 8: the three whole slots, leave (1, 2), enter (4 ..), gap (1, 2, 6 ..)
    assert pack.terms_per_step == [5, 5, 3, 4, 4, 5, 5, 5] and pack.num_terms == 36
    _, _, _, cnt = R.rollout_reference(raw, pack.start, H, LAW, 'GC', 0.08, desired_speed=1.3)
    assert cnt.tolist() == pack.terms_per_step


def test_windows_without_a_carried_slot_hold_no_term():
    from piml_amd.calibrate import pack_windows
    base = R.flow_clip(6, 10, TRUTH, 'GC', seed=2)
    # agents 0 .. 2 in the even frames, 3 .. 5 in the odd ones: present everywhere, never twice in a row
    raw = R.with_presence(base, {a: [(t, t + 1) for t in range(10) if (t + (a >= 3)) % 2] for a in range(6)})
    pack = pack_windows(raw, 4, desired_speed=1.3, device='cpu')
    assert pack.num_windows == 6 and pack.num_terms == 0 and pack.terms_per_step == [0] * 4
    assert not (pack.flags & R.CARRIED).any() and (pack.flags & R.PRESENT).sum() == 6 * 5 * 3
    loss, grad, sse, cnt = R.rollout_reference(raw, pack.start, 4, LAW, 'GC', 0.08, desired_speed=1.3)
    assert loss == 0.0 and not grad.any() and not sse.any() and not cnt.any()


def test_frames_of_sizes_hold_the_sizes_and_targets_asked_for():
    from piml_amd.calibrate import pack_clip
    sizes = [1, 2, 63, 64, 65, 66, 70]
    raw, target = R.frames_of_sizes(sizes, TRUTH, 'GC', seed=5, finite_targets={4: 3, 6: 0})
    present = torch.isfinite(raw.position).all(-1)
    assert present[:len(sizes)].sum(1).tolist() == sizes
    pack = pack_clip(raw, frames=range(len(sizes)), desired_speed=1.3, target=target, device='cpu')
    off = pack.offsets.tolist()
    assert [b - a for a, b in zip(off, off[1:])] == sizes
    # lane form up to 64 agents a frame, wave form above; frame 4 keeps 3 targets, frame 6 none
    assert pack.small_focal.numel() == 1 + 2 + 63 + 64 and pack.big_focal.numel() == 3 + 66
    assert pack.big_focal.tolist()[:3] == [off[4], off[4] + 1, off[4] + 2]
    full = R.flow_clip(70, len(sizes) + 1, TRUTH, 'GC', seed=5)
    fin = torch.isfinite(pack.target).all(-1)
    assert torch.equal(pack.target[fin], full.velocity[1:][pack.frame[fin], pack.agent[fin]])
    wave, lane = R.as_wave(pack), R.as_lane(pack)
    both = sorted(pack.small_focal.tolist() + pack.big_focal.tolist())
    assert wave.big_focal.tolist() == both and wave.small_focal.numel() == 0 and wave.big_focal.dtype == torch.int32
    assert lane.small_focal.tolist() == both and lane.big_focal.numel() == 0
    assert pack.small_focal.numel() == 130                                   # the editors copy


def test_window_editors_rebuild_the_big_lists():
    from piml_amd.calibrate import pack_windows
    base = R.flow_clip(66, 14, TRUTH, 'GC', seed=4)
    # 66 agents in frames 0 .. 4, 60 from frame 5 on: the windows from 0 and 3 hold 66 slots, those from 6 and 9 hold 60
    raw = R.with_presence(base, {a: [(5, 14)] for a in range(60, 66)})
    pack = pack_windows(raw, 4, stride=3, desired_speed=1.3, device='cpu')
    assert pack.start == [0, 3, 6, 9] and pack.slot_count == [66, 66, 60, 60]
    assert pack.small_windows.tolist() == [2, 3] and pack.big_windows.tolist() == [0, 1]
    assert pack.big_base.tolist() == [0, 66] and pack.big_slots == 132
    big = R.as_big(pack)
    assert big.small_windows.numel() == 0 and big.big_windows.tolist() == [0, 1, 2, 3]
    assert big.big_base.tolist() == [0, 66, 132, 192] and big.big_slots == 252
    assert big.big_windows.dtype == torch.int32 and big.big_base.dtype == torch.int32
    s, b = R.only_small(pack), R.only_big(pack)
    assert s.small_windows.tolist() == [2, 3] and s.big_windows.numel() == 0 and s.big_slots == 0
    assert b.big_windows.tolist() == [0, 1] and b.small_windows.numel() == 0 and b.big_base.tolist() == [0, 66]
    assert pack.big_slots == 132 and pack.small_windows.tolist() == [2, 3]
    with pytest.raises(AssertionError):
        R.with_windows(pack, [0], [])                                        # 66 slots are no small window
