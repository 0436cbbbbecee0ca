"""GPU: the MLAPM calibration (piml_mlapm_fit_loss_grad, piml_amd.calibrate) against the reference's own autograd, a
float64 restatement, the forward kernel, itself, and a scene with known constants."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from mlapm_fit_ref import ucy_reference

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


def evaluate(pack, params, version, dt, radius=0.3):
    from piml_amd import ops
    prm = torch.tensor([float(params[k]) for k in NAMES], dtype=torch.float32, device=DEV)
    loss, grad = ops.mlapm_fit_loss_grad(pack, prm, version, dt, radius)
    return float(loss.item()), grad.double().cpu().numpy()


@pytest.mark.parametrize('version', ['raw', 'GC'])
def test_loss_and_gradient_match_the_reference_autograd(version):
    from piml_amd.calibrate import pack_clip
    g = golden('mlapm_fit')
    raw = load(GC_CLIP)
    pack = pack_clip(raw, frames=[int(f) for f in g['frames']], device=DEV)
    for k in range(2):
        tag = f'{version}_{k}'
        assert pack.num_focal == int(g[f'count_{tag}'])
        params = dict(zip(NAMES, g[f'params_{tag}']))
        loss, grad = evaluate(pack, params, version, float(g['dt']), float(g['radius']))
        want, gw, scale = float(g[f'loss_{tag}']), g[f'grad_{tag}'], g[f'grad_scale_{tag}']
        assert abs(loss - want) <= 1e-5 * want, (tag, loss, want)
        for q, name in enumerate(NAMES):
            if scale[q] == 0:
                assert grad[q] == 0.0, (tag, name, grad[q])          # a constant the variant does not use
            else:
                assert abs(grad[q] - gw[q]) <= 1e-5 * scale[q], (tag, name, grad[q], gw[q], scale[q])


def test_ucy_matches_a_float64_restatement():
    from piml_amd.calibrate import pack_clip
    raw = load(UCY_CLIP)
    pack = pack_clip(raw, frames=range(100, 140), device=DEV)
    dt = raw.time_unit
    for params in (MAIN_MLAPM, {'tau': 0.9, 'A': 3.0, 'B': -1.0, 'C': 0.4, 'D': 0.0, 'theta': 20.0}):
        loss, grad = evaluate(pack, params, 'UCY', dt)
        want, gw = ucy_reference(pack, params, dt, 0.3)
        assert abs(loss - want) <= 1e-5 * want
        assert grad[4] == 0.0                                          # D: not in the UCY law
        # each gradient against its own magnitude and the largest one's (a sum with cancellations)
        bar = 1e-5 * np.maximum(np.abs(gw), 1e-3 * np.abs(gw).max())
        assert (np.abs(grad - gw) <= bar + 1e-5 * np.abs(gw)).all(), (grad, gw)


@pytest.mark.parametrize('version', ['raw', 'GC', 'UCY'])
def test_loss_equals_the_forward_kernel_frame_by_frame(version):
    """The fit's predictions are MLAPM.step's: the loss from ops.mlapm_step(skip_absent=True), one frame at a time."""
    from piml_amd import ops
    from piml_amd.calibrate import pack_clip
    raw = load(GC_CLIP)
    frames = list(range(0, 700, 7))
    pack = pack_clip(raw, frames=frames, device=DEV)
    dt = raw.time_unit
    loss, _ = evaluate(pack, MAIN_MLAPM, version, dt)
    N = raw.num_pedestrians
    fr, ag = pack.frame.tolist(), pack.agent.tolist()
    st, v0, tg = pack.state, pack.desired_speed, pack.target
    total, count = 0.0, 0
    off = pack.offsets.cpu().tolist()
    for f in range(len(frames)):
        a, b = off[f], off[f + 1]
        idx = torch.tensor(ag[a:b], device=DEV)
        p = torch.full((N, 2), float('nan'), device=DEV)
        v = torch.zeros(N, 2, device=DEV)
        d = torch.zeros(N, 2, device=DEV)
        s = torch.ones(N, device=DEV)
        p[idx], v[idx], d[idx], s[idx] = st[a:b, :2], st[a:b, 2:], pack.destination[a:b], v0[a:b]
        pred = ops.mlapm_step(p, v, s, d, dt, 0.3, version=version, skip_absent=True, **MAIN_MLAPM)[idx]
        t = tg[a:b]
        fin = torch.isfinite(t).all(-1)
        total += float(((pred[fin].double() - t[fin].double()) ** 2).sum())
        count += int(fin.sum())
    assert all(fr[i] == frames[f] for f in range(len(frames)) for i in range(off[f], off[f + 1]))
    want = total / count
    assert abs(loss - want) <= 1e-6 * want, (loss, want)


def test_deterministic_and_graph_equals_eager():
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, pack_clip
    raw = load(GC_CLIP)
    pack = pack_clip(raw, frames='100:400', device=DEV)
    prm = torch.tensor([MAIN_MLAPM[k] for k in NAMES], dtype=torch.float32, device=DEV)
    l1, g1 = (x.clone() for x in ops.mlapm_fit_loss_grad(pack, prm, 'GC', raw.time_unit, 0.3))
    l2, g2 = ops.mlapm_fit_loss_grad(pack, prm, 'GC', raw.time_unit, 0.3)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    kw = dict(version='GC', init=MAIN_MLAPM, steps=61, graph_steps=20)
    graph = calibrate_mlapm(pack, use_graph=True, **kw)
    eager = calibrate_mlapm(pack, use_graph=False, **kw)
    assert graph.params == eager.params and graph.history == eager.history and graph.final_loss == eager.final_loss
    assert graph.final_loss < graph.initial_loss


def circle_scene(truth, N=64, steps=160, dt=0.08, radius=0.3, seed=0):
    """The antipodal circle of src/main_mlapm.py with N agents, simulated by MLAPM.rollout at known constants."""
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    g = torch.Generator().manual_seed(seed)
    a = torch.linspace(0, 2 * math.pi * (1 - 1.0 / N), N)
    p = torch.stack([10 * a.cos(), 10 * a.sin()], -1)
    v = torch.rand(N, 2, generator=g)
    dest = -p
    model = MLAPM(version='GC', **truth)
    tp, tv = model.rollout(p.to(DEV), v.to(DEV), torch.full((N, 1), 1.5, device=DEV), dest.to(DEV), dt, radius, steps=steps)
    tp, tv = tp.cpu(), tv.cpu()
    # an agent within `radius` of its destination in a frame t >= 1 is no source for frame t + 1 (the rollout's rule; it is
    # NaN from t + 1 on): in the clip it is absent from frame t on
    gone = torch.norm(tp - dest, dim=-1) < radius
    gone[0] = False
    nan = torch.tensor(float('nan'))
    tp, tv = torch.where(gone.unsqueeze(-1), nan, tp), torch.where(gone.unsqueeze(-1), nan, tv)
    return RawData(position=tp, velocity=tv, destination=dest.expand(steps + 1, N, 2).clone(), meta_data={'time_unit': dt})


def test_calibration_recovers_known_constants():
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, pack_clip
    truth = dict(MAIN_MLAPM)
    raw = circle_scene(truth)
    pack = pack_clip(raw, desired_speed=1.5, device=DEV)
    assert pack.num_focal > 5000
    off = {'tau': 1.25, 'A': 0.75, 'B': 1.2, 'C': 0.78, 'D': 1.25, 'theta': 0.8}
    init = {k: truth[k] * off[k] for k in NAMES}
    # every constant moves the loss at the start: the scene exercises every term
    prm = torch.tensor([init[k] for k in NAMES], dtype=torch.float32, device=DEV)
    loss0, grad0 = ops.mlapm_fit_loss_grad(pack, prm, 'GC', 0.08, 0.3)
    sens = (grad0.double().abs() * prm.double().abs() / loss0).cpu().numpy()
    assert (sens > 0.02).all(), dict(zip(NAMES, sens))
    res = calibrate_mlapm(pack, version='GC', init=init, steps=1500, lr=0.03)
    for k in NAMES:
        if k == 'theta':
            assert abs(res.params[k] - truth[k]) <= 0.5, (k, res.params)
        else:
            assert abs(res.params[k] - truth[k]) <= 0.02 * abs(truth[k]), (k, res.params)
    assert res.final_loss <= 1e-4 * res.initial_loss, (res.initial_loss, res.final_loss)


def test_fit_on_the_gc_clip_and_cli(tmp_path):
    from piml_amd.calibrate import calibrate_mlapm, pack_clip
    from piml_amd.models.mlapm import MLAPM
    raw = load(GC_CLIP)
    pack = pack_clip(raw, frames='0:500', device=DEV)
    res = calibrate_mlapm(pack, version='GC', init=MAIN_MLAPM, steps=200)
    assert res.final_loss < 0.9 * res.initial_loss and len(res.history) == 200
    out = str(tmp_path / 'params.json')
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.calibrate', '--data',
                        os.path.join(REPO, 'tests', 'golden', 'data', GC_CLIP), '--version', 'GC', '--fit', 'A,B,theta',
                        '--frames', '0:500', '--valid_frames', '500:700', '--steps', '100', '--out', out],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'held-out loss' in p.stdout and 'loss' in p.stdout
    with open(out) as fh:
        params = json.load(fh)
    assert params['version'] == 'GC' and params['tau'] == MAIN_MLAPM['tau'] and params['C'] == pytest.approx(0.2)
    model = MLAPM(**params)
    t = 300
    m = torch.isfinite(raw.position[t]).all(-1) & (raw.mask_v[t] != 0)
    v = model.step(raw.position[t][m].to(DEV), raw.velocity[t][m].to(DEV), torch.full((int(m.sum()), 1), 1.3, device=DEV),
                   raw.destination[t][m].to(DEV), raw.time_unit)
    assert torch.isfinite(v).all()
