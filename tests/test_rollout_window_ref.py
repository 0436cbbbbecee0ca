"""CPU: the float64 restatement of a rollout window (tests/rollout_window_ref.py) pinned on what it restates -- its gathered
features on the float32 oracle's (same indices; one float32 rounding apart), its frame step on the torch-operator branch of
BaseSimulator._training_rollout_frames run in float64 on the golden `rollout` batch (the fixture holds no per-frame state),
its tail on the literal reference expression -- and the scenes of tests/test_rollout_window_gpu.py checked for the margin the
comparison needs: no agent within 1e-3 of the 0.5 m waypoint radius in any frame."""
import numpy as np
import pytest
import torch

from conftest import golden
import rollout_window_ref as R


def test_gathered_features_equal_the_oracle(oracle):
    from piml_amd.scenes import synthetic_gc_scene
    C, N, M = 3, 57, 40
    sc = synthetic_gc_scene(N, M, seed=5, channels=C)
    rng = np.random.default_rng(5)
    acc = (0.3 * rng.standard_normal((C, N, 2))).astype(np.float32)
    acc[0, 3, 1] = np.nan                                                   # read as 0
    args = [sc['position'], sc['velocity'], acc, sc['destination']]
    pf, of, df, pi, oi, _, _ = oracle.relfeat_fwd(*[x[:, None] for x in args], sc['obstacles'], return_index=True)
    assert (pi >= 0).any() and (pi < 0).any() and (oi >= 0).any() and np.isnan(sc['position']).any()
    t64 = [torch.from_numpy(x).double() for x in args]
    got = R.gathered_features(*t64, torch.from_numpy(sc['obstacles']).double(), torch.from_numpy(sc['desired_speed']).double(),
                              torch.from_numpy(pi[:, 0]), torch.from_numpy(oi[:, 0]))
    v0 = np.nan_to_num(sc['velocity'])
    want_sf = np.concatenate((df[:, 0], v0, np.nan_to_num(acc), sc['desired_speed']), -1)
    for name, a, b in (('ped', got[0], pf[:, 0]), ('obs', got[1], of[:, 0]), ('self', got[2], want_sf)):
        a, b = a.numpy(), b.astype(np.float64)
        # the oracle forms every entry with ONE float32 subtraction of the same float32 inputs: half an ulp, 2^-24 relative
        assert np.all(np.abs(a - b) <= 2.0 ** -24 * np.abs(a) + 1e-300), name
        assert a.shape == b.shape


def test_frame_step_equals_the_torch_operator_branch_in_float64():
    """src/models/simulators.py:741-769 as piml_amd/models/simulators.py states it on torch operators (the branch the fused frame
    step replaces), in float64, on frames 0 -> 1 and 3 -> 4 (no injection behind the last frame) of the golden training batch."""
    from piml_amd.models.simulators import BaseSimulator, _gather_waypoints
    g = golden('rollout')
    f = lambda k: torch.from_numpy(g['train_pinnsf_m/' + k])
    pos, vel, acc, dst = [f(k).double() for k in ('position', 'velocity', 'acceleration', 'destination')]
    didx, dnum, way = f('dest_idx'), f('dest_num'), f('waypoints').double()
    new_flag = (f('mask_p') - f('mask_p_pred')).long() == 1
    C, T, N = pos.shape[:3]
    dt = float(g['train_pinnsf_m/time_unit'])
    gen = torch.Generator().manual_seed(1)
    a_next = torch.randn(C, N, 2, generator=gen, dtype=torch.float64)
    a_next[0, 0, 0] = float('nan')
    assert new_flag[:, 1:].any() and pos.isnan().any()
    for t in (0, T - 2, T - 1):
        p_cur, v_cur, a_cur, dest_cur, dest_idx = pos[:, t], vel[:, t], acc[:, t], dst[:, t], didx[:, t]
        inject = t < T - 1
        truth = tuple(x[:, t + 1] for x in (pos, vel, acc, dst, didx)) if inject else None
        got = R.frame_step(p_cur, v_cur, a_cur, a_next, dest_cur, dest_idx, way, dnum, dt, new_flag[:, t + 1] if inject else None, truth)
        # the branch, statement by statement
        v_next = v_cur + a_cur * dt
        p_next = p_cur + v_cur * dt
        near = torch.norm(p_cur - dest_cur, p=2, dim=-1) < 0.5
        idx = dest_idx + near.long()
        idx = idx - (idx > dnum - 1).long()
        dest_n = _gather_waypoints(way, idx)
        p_n, v_n, a_n = p_next, v_next, a_next
        if inject:
            new = new_flag[:, t + 1]
            p_n = BaseSimulator._inject(new, p_n, pos[:, t + 1])
            v_n = BaseSimulator._inject(new, v_n, vel[:, t + 1])
            a_n = BaseSimulator._inject(new, a_n, acc[:, t + 1])
            dest_n = BaseSimulator._inject(new, dest_n, dst[:, t + 1])
            idx = BaseSimulator._inject(new, idx, didx[:, t + 1])
        v_n, a_n = torch.nan_to_num(v_n, nan=0.0), torch.nan_to_num(a_n, nan=0.0)       # get_relative_features, in place
        for a, b in zip(got[:5], (p_n, v_n, a_n, dest_n, idx)):
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_agent_norm_tail_equals_the_reference_expression():
    """quirk Q2: torch.norm(dest, dim=1) of channelled (C, N, 2) input is a norm over the AGENTS, per component."""
    gen = torch.Generator().manual_seed(2)
    C, N = 3, 9
    sf = torch.randn(C, N, 7, generator=gen, dtype=torch.float64)
    sf[1, :, 0] = 0.0
    sf.requires_grad_(True)
    ap, ao = torch.randn(C, N, 6, 2, generator=gen, dtype=torch.float64), torch.randn(C, N, 10, 2, generator=gen, dtype=torch.float64)
    got = R.agent_norm_tail(ap, ao, sf, 2.0)
    d = sf[..., :2]
    t = torch.norm(d.detach(), p=2, dim=1, keepdim=True)
    t = torch.where(t == 0, t + 0.1, t)
    want = ap.sum(2) + ao.sum(2) + (sf[..., 6:7] * d / t - sf[..., 2:4]) / 2.0
    assert torch.allclose(got, want, rtol=1e-14, atol=1e-14)
    gs, = torch.autograd.grad(got.sum(), sf)
    assert torch.isfinite(gs).all() and float(gs[1, :, 0].abs().max()) > 0           # the 0 -> 0.1 branch: finite, d/0.1


@pytest.mark.parametrize('name,t_start', [(n, 0) for n in sorted(R.SHAPES)] + [('n257', 1), ('n300', 1)])
def test_scenes_keep_clear_of_the_waypoint_radius(oracle, name, t_start):
    """The float64 window on the CPU (indices from the float32 oracle) for every scene of the GPU tests: every frame switches
    somebody's waypoint or nobody's knowingly -- no agent within 1e-3 of the 0.5 m radius -- and the scene holds what the GPU
    cases are there for (injections, a closed gate, NaN agents, the injected NaN velocity)."""
    C, T, N, M, seed, wps, gate = R.SHAPES[name]
    case32 = R.make_case(C, T, N, M, seed, wps, gate)
    case = R.case_to(case32, 'cpu', torch.float64)
    p, v, a, dest = [case[k][:, t_start] for k in ('position', 'velocity', 'acceleration', 'destination')]
    sel = R.oracle_select(case32)
    pi, oi = sel(t_start, p, v, a, dest)
    feats0 = R.gathered_features(p, v, a, dest, case['obstacles'], case['self_features'][:, t_start, :, 6:], pi, oi)
    for kind in ('ksum', 'sum'):
        out = R.window(case, p, v, a, feats0, case['Wp'], case['Wo'], kind, t_start, sel)
        margin = min(float(m.min()) for m in out['margin'] if m.numel())
        assert margin > 1e-3, f'{name}: an agent {margin:.2e} from the waypoint radius -- change the seed'
        last = out['frames'][-1]
        assert torch.isfinite(last[1]).all() and torch.isfinite(last[2]).all()
    new = (case['mask_p'] - case['mask_p_pred']) == 1
    if N > 1:
        assert sum(out['near']) > 0                                                    # somebody does switch waypoints
        frac = float(new[:, 1:].float().mean())
        assert 0.1 < frac < 0.6 and case['position'].isnan().any()
        assert (case['velocity'].isnan() & ~case['position'].isnan()).any()           # the injected NaN component
        assert not gate or not bool(case['mask_p_pred'][:, T - 2].any())                # the closed gate
