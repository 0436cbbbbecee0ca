"""GPU: the MLAPM rollout calibration (piml_mlapm_rollout_fit_loss_grad, calibrate_mlapm(horizon=H)) against the
reference's own autograd, a float64 restatement (UCY, frames of more than 64 agents), the one-step kernel at H = 1,
itself, and scenes with known constants."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from mlapm_fit_ref import check_against, rollout_reference

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
MAIN_MLAPM = {'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
UCY_CLIP = 'UCY_Dataset_time162-216_timeunit0.08.npy'


def load(name):
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(REPO, 'tests', 'golden', 'data', name))
    return raw


def evaluate(pack, params, version, dt, radius=0.3, decay=1.0):
    from piml_amd import ops
    prm = torch.tensor([float(params[k]) for k in NAMES], dtype=torch.float32, device=DEV)
    ps = torch.empty(2 * pack.horizon, dtype=torch.float64, device=DEV)
    loss, grad = ops.mlapm_rollout_fit_loss_grad(pack, prm, version, dt, radius, decay, per_step=ps)
    return float(loss.item()), grad.double().cpu().numpy(), ps.cpu().numpy()


@pytest.mark.parametrize('version', ['raw', 'GC'])
def test_loss_and_gradient_match_the_reference_autograd(version):
    from piml_amd.calibrate import pack_windows
    g = golden('mlapm_rollout_fit')
    raw = load(GC_CLIP)
    H, stride = int(g['horizon']), int(g['stride'])
    a, b = (int(x) for x in g['frames'])
    pack = pack_windows(raw, H, frames=f'{a}:{b}', stride=stride, device=DEV)
    assert pack.start == [int(x) for x in g['starts']] and pack.big_windows.numel() == 0
    worst = 0.0
    for k in range(2):
        for q, decay in enumerate(g['decays']):
            tag = f'{version}_{k}_{q}'
            assert pack.num_terms == int(g[f'count_{tag}'])
            params = dict(zip(NAMES, g[f'params_{tag}']))
            loss, grad, ps = evaluate(pack, params, version, float(g['dt']), float(g['radius']), float(decay))
            want, gw, scale = float(g[f'loss_{tag}']), g[f'grad_{tag}'], g[f'grad_scale_{tag}']
            assert abs(loss - want) <= 1e-5 * want, (tag, loss, want)
            assert np.array_equal(ps[H:], g[f'step_count_{tag}'])
            assert np.allclose(ps[:H], g[f'sse_{tag}'], rtol=1e-5, atol=0), (tag, ps[:H], g[f'sse_{tag}'])
            for i, name in enumerate(NAMES):
                if scale[i] == 0:
                    assert grad[i] == 0.0, (tag, name, grad[i])          # a constant the variant does not use
                else:
                    worst = max(worst, abs(grad[i] - gw[i]) / scale[i])
                    assert abs(grad[i] - gw[i]) <= 1e-5 * scale[i], (tag, name, grad[i], gw[i], scale[i])
    print(f'[rollout fit] {version}: worst gradient error {worst:.3g} of its scale')


def test_ucy_matches_a_float64_restatement():
    from piml_amd.calibrate import pack_windows
    raw = load(UCY_CLIP)
    dt = raw.time_unit
    pack = pack_windows(raw, 8, frames='100:149', stride=4, device=DEV)
    for params in (MAIN_MLAPM, {'tau': 0.9, 'A': 3.0, 'B': -1.0, 'C': 0.4, 'D': 0.0, 'theta': 20.0}):
        loss, grad, ps = evaluate(pack, params, 'UCY', dt)
        want, gw, sse, cnt = rollout_reference(raw, pack.start, 8, params, 'UCY', dt)
        assert grad[4] == 0.0                                          # D: not in the UCY law
        check_against(loss, grad, ps, want, gw, sse, cnt)


def test_horizon_one_is_dt_squared_times_the_one_step_fit():
    from piml_amd import ops
    from piml_amd.calibrate import _present_and_speed, pack_clip, pack_windows
    raw = load(GC_CLIP)
    dt = raw.time_unit
    pack = pack_windows(raw, 1, frames='100:400', device=DEV)
    assert pack.start == list(range(100, 399))
    P, _, _, present, _ = _present_and_speed(raw, None, 25)
    target = torch.full_like(P, float('nan'))
    target[:-1] = torch.where(present[1:].unsqueeze(-1), (P[1:] - P[:-1]) / dt, target[1:])
    fit = pack_clip(raw, frames='100:399', target=target, device=DEV)
    assert fit.num_focal == pack.num_terms
    for version in ('raw', 'GC', 'UCY'):
        prm = torch.tensor([MAIN_MLAPM[k] for k in NAMES], dtype=torch.float32, device=DEV)
        l1, g1 = ops.mlapm_rollout_fit_loss_grad(pack, prm, version, dt, 0.3)
        l0, g0 = ops.mlapm_fit_loss_grad(fit, prm, version, dt, 0.3)
        l1, l0 = float(l1.item()), float(l0.item()) * dt * dt
        g1, g0 = g1.double().cpu().numpy(), g0.double().cpu().numpy() * dt * dt
        assert abs(l1 - l0) <= 1e-5 * l0, (version, l1, l0)
        assert np.allclose(g1, g0, rtol=1e-5, atol=1e-5 * np.abs(g0).max()), (version, g1, g0)


def circle_scene(truth, N=64, steps=160, dt=0.08, radius=0.3, seed=0, ring=10.0):
    """The antipodal circle of src/main_mlapm.py with N agents on a circle of `ring` metres, simulated by MLAPM.rollout
    at known constants (the helper of tests/test_mlapm_fit_gpu.py, restated, with the ring's radius as an argument)."""
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    g = torch.Generator().manual_seed(seed)
    a = torch.linspace(0, 2 * math.pi * (1 - 1.0 / N), N)
    p = torch.stack([ring * a.cos(), ring * a.sin()], -1)
    v = torch.rand(N, 2, generator=g)
    dest = -p
    model = MLAPM(version='GC', **truth)
    tp, tv = model.rollout(p.to(DEV), v.to(DEV), torch.full((N, 1), 1.5, device=DEV), dest.to(DEV), dt, radius, steps=steps)
    tp, tv = tp.cpu(), tv.cpu()
    gone = torch.norm(tp - dest, dim=-1) < radius
    gone[0] = False
    nan = torch.tensor(float('nan'))
    tp, tv = torch.where(gone.unsqueeze(-1), nan, tp), torch.where(gone.unsqueeze(-1), nan, tv)
    return RawData(position=tp, velocity=tv, destination=dest.expand(steps + 1, N, 2).clone(), meta_data={'time_unit': dt})


def test_frames_of_more_than_64_agents_match_a_float64_restatement():
    from piml_amd.calibrate import pack_windows
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    # the antipodal circle of 256 agents, spaced as the 64 of the 10 m circle: on the 10 m circle they stand 0.25 m apart,
    # every pair inside the UCY collision distance, and the rollouts are chaotic (a 1e-7 relative change of the recorded
    # positions moves the float64 gradient by more than 10 %), which no float32 / float64 comparison can resolve
    raw = circle_scene(MAIN_MLAPM, N=256, steps=40, ring=40.0)
    pack = pack_windows(raw, 8, frames='10:35', stride=8, desired_speed=1.5, device=DEV)
    assert pack.small_windows.numel() == 0 and min(pack.slot_count) == 256 and pack.num_windows == 3
    params = {'tau': 0.7, 'A': 5.0, 'B': -2.0, 'C': 0.3, 'D': -0.2, 'theta': 40.0}
    for version in ('raw', 'GC'):
        loss, grad, ps = evaluate(pack, params, version, 0.08)
        want, gw, sse, cnt = rollout_reference(raw, pack.start, 8, params, version, 0.08, desired_speed=1.5)
        check_against(loss, grad, ps, want, gw, sse, cnt)
    # an open-world GC clip simulated by the law, where its frames hold more than 64 agents
    res = MLAPM(version='GC', **MAIN_MLAPM).simulate_scenario(gc_scenario().to(DEV), 260, seed=4)
    n = res.num_agents
    sim = res.to_raw_data()
    present = torch.isfinite(sim.position).all(-1) & (sim.mask_v != 0)
    t0 = int(torch.nonzero(present.sum(1) > 64)[0])
    assert t0 + 30 < 260, t0
    frames = f'{t0}:{t0 + 25}'
    pack = pack_windows(sim, 8, frames=frames, stride=8, desired_speed=res.desired_speed[:n], device=DEV)
    assert int(present[t0:t0 + 25].sum(1).min()) > 64 and pack.small_windows.numel() == 0
    for params in (MAIN_MLAPM, {'tau': 0.7, 'A': 5.0, 'B': -2.0, 'C': 0.3, 'D': -0.2, 'theta': 40.0}):
        loss, grad, ps = evaluate(pack, params, 'GC', sim.time_unit)
        want, gw, sse, cnt = rollout_reference(sim, pack.start, 8, params, 'GC', sim.time_unit,
                                               desired_speed=res.desired_speed[:n].cpu())
        if params is MAIN_MLAPM:
            assert want < 1e-9 and loss < 1e-9, (loss, want)           # the clip's own law: rounding only
        else:
            check_against(loss, grad, ps, want, gw, sse, cnt)


def test_deterministic_and_graph_equals_eager():
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, pack_windows
    raw = load(GC_CLIP)
    pack = pack_windows(raw, 8, frames='100:300', device=DEV)
    big = pack_windows(circle_scene(MAIN_MLAPM, N=96, steps=30), 8, desired_speed=1.5, device=DEV)
    for pk, dt in ((pack, raw.time_unit), (big, 0.08)):
        prm = torch.tensor([MAIN_MLAPM[k] for k in NAMES], dtype=torch.float32, device=DEV)
        ps1, ps2 = (torch.empty(16, dtype=torch.float64, device=DEV) for _ in range(2))
        l1, g1 = (x.clone() for x in ops.mlapm_rollout_fit_loss_grad(pk, prm, 'GC', dt, 0.3, 0.9, per_step=ps1))
        l2, g2 = ops.mlapm_rollout_fit_loss_grad(pk, prm, 'GC', dt, 0.3, 0.9, per_step=ps2)
        assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(ps1, ps2)
    kw = dict(version='GC', init=MAIN_MLAPM, steps=41, graph_steps=20, horizon=8)
    graph = calibrate_mlapm(pack, use_graph=True, **kw)
    eager = calibrate_mlapm(pack, use_graph=False, **kw)
    assert graph.params == eager.params and graph.history == eager.history and graph.final_loss == eager.final_loss
    assert graph.final_loss < graph.initial_loss and graph.horizon == 8


def test_recovers_known_constants_of_a_simulated_scene():
    from piml_amd.calibrate import calibrate_mlapm, mlapm_rollout_fit_loss, pack_windows
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    truth = {'tau': 0.5, 'A': 6.5, 'B': -2.5, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
    res = MLAPM(version='GC', **truth).simulate_scenario(gc_scenario().to(DEV), 200, seed=11)
    n = res.num_agents
    pack = pack_windows(res.to_raw_data(), 8, desired_speed=res.desired_speed[:n], device=DEV)
    at, _ = mlapm_rollout_fit_loss(pack, truth, 'GC')
    init = {**truth, 'tau': truth['tau'] * 0.85, 'A': truth['A'] * 1.2, 'B': truth['B'] * 0.8}
    moved, _ = mlapm_rollout_fit_loss(pack, init, 'GC')
    assert at < 1e-10 and moved >= 1e4 * max(at, 1e-14), (at, moved)
    fit = calibrate_mlapm(pack, 'GC', init=init, fit=('tau', 'A', 'B'), steps=800, horizon=8)
    err = {k: abs(fit.params[k] / truth[k] - 1) for k in ('tau', 'A', 'B')}
    print(f'[rollout fit] scene: loss at truth {at:.3g}, start {moved:.3g}, fitted {fit.final_loss:.3g}, errors {err}')
    assert max(err.values()) <= 0.02, err


def test_recovers_the_constants_of_the_circle():
    """All six constants fitted on the 64-agent antipodal circle from the one-step test's 20-30 % offsets.  tau, A, B and
    theta come back to the one-step test's tolerances.  C and D (the cosine of the relative velocity) move the rollout
    positions little and come back only part of the way in the same budget: on the MI355X C -7 %, D -12 % from -22 % and
    +25 %, so for them the test asserts that the error shrinks."""
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, pack_windows
    truth = dict(MAIN_MLAPM)
    raw = circle_scene(truth)
    pack = pack_windows(raw, 4, frames='0:60', desired_speed=1.5, device=DEV)
    assert pack.num_terms > 5000 and pack.big_windows.numel() == 0
    off = {'tau': 1.25, 'A': 0.75, 'B': 1.2, 'C': 0.78, 'D': 1.25, 'theta': 0.8}
    init = {k: truth[k] * off[k] for k in NAMES}
    prm = torch.tensor([init[k] for k in NAMES], dtype=torch.float32, device=DEV)
    loss0, grad0 = ops.mlapm_rollout_fit_loss_grad(pack, prm, 'GC', 0.08, 0.3)
    sens = (grad0.double().abs() * prm.double().abs() / loss0).cpu().numpy()
    assert (sens > 0.02).all(), dict(zip(NAMES, sens))
    res = calibrate_mlapm(pack, version='GC', init=init, steps=3000, lr=0.03, horizon=4)
    print(f'[rollout fit] circle: {res.initial_loss:.3g} -> {res.final_loss:.3g}, {res.params}')
    for k in ('tau', 'A', 'B'):
        assert abs(res.params[k] - truth[k]) <= 0.02 * abs(truth[k]), (k, res.params)
    assert abs(res.params['theta'] - truth['theta']) <= 0.5, res.params
    for k in ('C', 'D'):
        assert abs(res.params[k] - truth[k]) < abs(init[k] - truth[k]) * 0.6, (k, res.params)
    assert res.final_loss <= 1e-2 * res.initial_loss, (res.initial_loss, res.final_loss)


def test_fit_on_the_gc_clip_and_cli(tmp_path):
    from piml_amd.calibrate import calibrate_mlapm, mlapm_rollout_fit_loss, pack_windows
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    raw = load(GC_CLIP)
    pack = pack_windows(raw, 16, frames='0:500', device=DEV)
    res = calibrate_mlapm(pack, version='GC', init=MAIN_MLAPM, steps=200, horizon=16)
    assert len(res.history) == 200 and res.final_loss < res.initial_loss
    valid = pack_windows(raw, 16, frames='500:700', device=DEV)
    before, _ = mlapm_rollout_fit_loss(valid, MAIN_MLAPM, 'GC')
    after, _ = mlapm_rollout_fit_loss(valid, res.params, 'GC')
    print(f'[rollout fit] GC clip H = 16: train {res.initial_loss:.4g} -> {res.final_loss:.4g}, '
          f'held-out {before:.4g} -> {after:.4g}')
    assert after < before, (before, after)
    out = str(tmp_path / 'params.json')
    env = dict(os.environ, PYTHONPATH=REPO)
    clip = os.path.join(REPO, 'tests', 'golden', 'data', GC_CLIP)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.calibrate', '--data', clip, clip, '--version', 'GC',
                        '--fit', 'A,B,theta', '--frames', '0:500', '--valid_frames', '500:700', '--horizon', '16',
                        '--stride', '2', '--time_decay', '0.95', '--steps', '60', '--out', out],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'held-out rollout loss' in p.stdout and 'RMSE at k = 16' in p.stdout
    with open(out) as fh:
        params = json.load(fh)
    assert params['version'] == 'GC' and params['tau'] == MAIN_MLAPM['tau'] and params['C'] == pytest.approx(0.2)
    sim = MLAPM(**params).simulate_scenario(gc_scenario().to(DEV), 20, seed=1)
    assert torch.isfinite(sim.position[:, :sim.num_agents]).any()
