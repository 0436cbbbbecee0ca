"""GPU: open-world scenes driven by the MLAPM law (piml_scenario_step_mlapm, MLAPM.simulate_scenario / simulate_ensemble):
every frame one MLAPM step of the present agents (against piml_mlapm_step_fwd and a torch restatement of mlapm.py), the
network's arrivals, members bitwise the single run, captured == eager, a calibration round trip, the argument errors
and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCENES = ('gc', 'crosswalk', 'four_directional_square', 'basic_unit1', 'basic_unit2', 'basic_unit3')
SEEDS = [0, 5, (1 << 33) + 7]
LAW = dict(tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)       # main_mlapm.py:16
FIELDS = ('position', 'velocity', 'acceleration', 'destination', 'mask_p', 'waypoints', 'desired_speed', 'spawn_count')


def make(name, **kw):
    from piml_amd.scenarios import SCENARIOS
    return SCENARIOS[name](**kw).to(DEV)


def mlapm(version='GC', **kw):
    from piml_amd.models.mlapm import MLAPM
    return MLAPM(version=version, **{**LAW, **kw})


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in FIELDS) and \
        a.spawned == b.spawned and a.dropped == b.dropped


def _step_fwd(p, v, v0, d, version, dt, radius=0.3):
    """piml_mlapm_step_fwd with skip_absent: (action, force) -- the kernel pinned to the reference's goldens."""
    from piml_amd import _lib, ops
    p, v, d, v0 = (x.contiguous() for x in (p, v, d, v0))
    act, frc = torch.empty_like(p), torch.empty_like(p)
    L = LAW
    _lib.check(_lib.lib().piml_mlapm_step_fwd(p.data_ptr(), v.data_ptr(), v0.data_ptr(), d.data_ptr(), p.shape[0],
                                              ops.MLAPM_VARIANTS[version], L['tau'], L['A'], L['B'], L['C'], L['D'],
                                              L['theta'], radius, dt, 1, act.data_ptr(), frc.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), 'piml_mlapm_step_fwd')
    return act, frc


def _restated(p, v, v0, d, version, dt, radius=0.3):
    """src/models/mlapm.py:10-58 in float64 on compacted agents; the discrete decisions (view, rotation sign, UCY
    collision) in float32 as the reference makes them, with the coll.unsqueeze(-1) fix."""
    import torch.nn.functional as F
    L = LAW
    p32, v32, d32 = p.float(), v.float(), d.float()
    P, V, Dst, V0 = p.double(), v.double(), d.double(), v0.double().reshape(-1, 1)
    ed = F.normalize(Dst - P, dim=-1)
    force = (V0 * ed - V) / L['tau']
    vr = P.view(1, -1, 2) - P.view(-1, 1, 2)
    vr32 = p32.view(1, -1, 2) - p32.view(-1, 1, 2)
    r = vr.norm(dim=2, keepdim=True)
    view = (torch.einsum('nk,nmk->nm', v32, vr32) > 0.).unsqueeze(-1).double()
    if version == 'raw':
        return V + (force - (view * L['A'] * (L['B'] * r).exp() * F.normalize(vr, dim=-1)).sum(1)) * dt
    ed32 = F.normalize(d32 - p32, dim=-1)
    sgn = -(vr32[:, :, 0] * ed32[:, None, 1] - vr32[:, :, 1] * ed32[:, None, 0]).sign().double()
    th = sgn * L['theta'] / 180 * np.pi
    th = torch.where(th == 0, torch.full_like(th, L['theta'] / 180 * np.pi), th)
    rot = torch.stack([th.cos(), -th.sin(), th.sin(), th.cos()], -1).view(*th.shape, 2, 2)
    direc = torch.einsum('NMij,NMj->NMi', rot, F.normalize(vr, dim=-1))
    vv = V.view(1, -1, 2) - V.view(-1, 1, 2)
    if version == 'GC':
        cos = F.cosine_similarity(vr, vv, dim=-1).unsqueeze(-1)
        g = (L['B'] * r + L['C'] * cos + L['D'] * r * cos).exp()
    else:
        vv32 = v32.view(1, -1, 2) - v32.view(-1, 1, 2)
        coll = vr32.norm(dim=-1) < radius * 2
        coll |= (vr32 + vv32).norm(dim=-1) < radius * 2
        tmin = -(vr32 * vv32).sum(-1) / (vv32 * vv32).sum(-1)
        dmin = ((vr32 * vr32).sum(-1) - (vr32 * vv32).sum(-1) ** 2 / (vv32 * vv32).sum(-1)).sqrt()
        coll |= (tmin > 0) & (tmin < 1) & (dmin < radius * 2)
        c = coll.unsqueeze(-1).double()
        g = (L['B'] * r * c + L['C'] * c).exp()
    return V + (force - (view * L['A'] * g * direc).sum(1)) * dt


@pytest.mark.parametrize('name', ['gc', 'crosswalk'])
@pytest.mark.parametrize('version', ['raw', 'GC', 'UCY'])
def test_every_frame_is_one_mlapm_step(name, version):
    sc = make(name)
    T, dt = 200, float(sc.time_unit)
    res = mlapm(version).simulate_scenario(sc, T, seed=3)
    # all capacity rows, as the frame's own call would see them (slots not yet spawned are NaN and skipped)
    p, v, a, d, m = res.position, res.velocity, res.acceleration, res.destination, res.mask_p
    v0 = res.desired_speed
    checked, bitwise, worst = 0, True, [0.0, 0.0, 0.0]
    for t in range(T - 1):
        keep = (m[t] == 1) & (m[t + 1] == 1)
        if not bool(keep.any()):
            continue
        act, frc = _step_fwd(p[t], v[t], v0, d[t], version, dt)
        vn = act[keep]
        pn = p[t][keep] + vn * dt
        for j, (x, y) in enumerate(((v[t + 1][keep], vn), (p[t + 1][keep], pn), (a[t + 1][keep], frc[keep]))):
            worst[j] = max(worst[j], (x - y).abs().max().item())
            bitwise &= torch.equal(bits(x), bits(y))
        checked += int(keep.sum())
        if t in (10, 100, 190):                              # the float64 restatement on the compacted present agents
            pres = m[t] == 1
            ref = _restated(p[t][pres], v[t][pres], v0[pres], d[t][pres], version, dt)
            ok = keep[pres]
            assert (v[t + 1][pres][ok].double() - ref[ok]).abs().max().item() <= 1e-5, t
    assert checked > 1000
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6 and worst[2] <= 1e-5, worst
    assert bitwise                                           # the frame adds the same terms in the same order (mlapm.hpp)
    print(f'[mlapm scene] {name} {version}: {checked} agent steps, bitwise against piml_mlapm_step_fwd: {bitwise}, '
          f'max |dv| {worst[0]:.3g} |dp| {worst[1]:.3g} |da| {worst[2]:.3g}')


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


@pytest.mark.parametrize('name', SCENES)
def test_same_arrivals_as_the_network(sim, name):
    sc = make(name)
    T = 120
    net = sim.simulate_scenario(sc, T, seed=7)
    law = mlapm('GC').simulate_scenario(sc, T, seed=7)
    assert net.capacity == law.capacity and net.spawned == law.spawned and net.dropped == law.dropped
    assert torch.equal(net.spawn_count, law.spawn_count)
    for k in ('waypoints', 'desired_speed'):
        assert torch.equal(bits(getattr(net, k)), bits(getattr(law, k))), k
    assert torch.equal(net.state.exit_idx, law.state.exit_idx)
    n = law.num_agents
    on_net, on_law = net.mask_p[:, :n] == 1, law.mask_p[:, :n] == 1
    first = on_net.int().argmax(0)
    assert torch.equal(first, on_law.int().argmax(0))
    cols = torch.arange(n, device=first.device)
    assert torch.equal(bits(net.position[first, cols]), bits(law.position[first, cols]))


@pytest.mark.parametrize('name', SCENES)
def test_members_are_bitwise_the_single_run(name):
    sc = make(name)
    T, law = 200, mlapm('UCY' if name == 'crosswalk' else 'GC')
    ens = law.simulate_ensemble(sc, T, SEEDS)
    for m, s in enumerate(SEEDS):
        one = law.simulate_scenario(sc, T, seed=s, capacity=ens.capacity)
        assert _same(ens.member(m), one), (name, s)


@pytest.mark.parametrize('version', ['GC', 'UCY'])
def test_captured_equals_eager(version):
    sc, law = make('gc'), mlapm(version)
    g = law.simulate_scenario(sc, 150, seed=2, use_graph=True)
    e = law.simulate_scenario(sc, 150, seed=2, use_graph=False)
    g2 = law.simulate_scenario(sc, 150, seed=2)
    assert _same(g, e) and _same(g, g2)
    ge = law.simulate_ensemble(sc, 150, [2, 4], use_graph=True)
    ee = law.simulate_ensemble(sc, 150, [2, 4], use_graph=False)
    assert _same(ge, ee)


def test_calibration_round_trip():
    from piml_amd.calibrate import calibrate_mlapm, mlapm_fit_loss, pack_clip
    sc = make('gc')
    P = {'tau': 0.5, 'A': 6.5, 'B': -2.5, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
    res = mlapm('GC', **P).simulate_scenario(sc, 200, seed=11)
    n = res.num_agents
    pack = pack_clip(res.to_raw_data(), desired_speed=res.desired_speed[:n])
    at, _ = mlapm_fit_loss(pack, P, 'GC')
    off = {**P, 'A': P['A'] * 1.1, 'B': P['B'] * 1.1}
    moved, _ = mlapm_fit_loss(pack, off, 'GC')
    assert at < 1e-10 and moved >= 1e4 * at, (at, moved)
    fit = calibrate_mlapm(pack, 'GC', init=off, fit=('tau', 'A', 'B'), steps=800)
    err = {k: abs(fit.params[k] / P[k] - 1) for k in ('tau', 'A', 'B')}
    print(f'[mlapm scene] calibration round trip: loss at P {at:.3g}, offset {moved:.3g}, fitted {fit.final_loss:.3g}, '
          f'relative errors {err}')
    assert max(err.values()) <= 2.2e-7, err                  # 3x the MI355X measurement (A 7.3e-8; tau, B exact)


def test_argument_errors():
    from piml_amd import _lib, ops_scenario
    sc = make('gc')
    st = ops_scenario.scenario_state(sc, 64, 10, seed=1)
    ops_scenario.scenario_step(st, init=True)
    torch.cuda.synchronize()
    before = [x.clone() for x in (st.p, st.v, st.p_res, st.spawned, st.t)]
    L, law = _lib.lib(), ops_scenario.mlapm_law()
    seeds = torch.tensor([1], device=DEV, dtype=torch.long)
    call = lambda lw, members=1, sd=seeds.data_ptr(), off=0, desc=st.desc: L.piml_scenario_step_mlapm(
        ctypes.byref(desc), None, members, sd, ctypes.byref(lw) if lw is not None else None, off, None)
    for field, val in (('variant', 3), ('variant', -1), ('tau', 0.0), ('tau', float('nan')), ('A', float('inf')),
                       ('B', float('nan')), ('C', float('inf')), ('D', float('nan')), ('theta_deg', float('inf')),
                       ('radius', 0.0), ('radius', -1.0)):
        bad = _lib.MlapmLaw.from_buffer_copy(law)
        setattr(bad, field, val)
        assert call(bad) == 1, (field, val)
    assert call(None) == 1 and call(law, members=0) == 1 and call(law, members=65536) == 1
    assert call(law, sd=None) == 1 and call(law, off=-1) == 1
    broken = _lib.Scenario.from_buffer_copy(st.desc)
    broken.spawn_cap = 9
    assert call(law, desc=broken) == 1
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(before, (st.p, st.v, st.p_res, st.spawned, st.t)))
    with pytest.raises(ValueError):
        mlapm('GC', tau=0.0).simulate_scenario(sc, 10)
    with pytest.raises(ValueError):
        mlapm('GC').simulate_scenario(sc, 10, radius=0.0)
    with pytest.raises(ValueError):
        mlapm('GC').simulate_ensemble(sc, 10, [])


def test_simulate_cli_mlapm_seeds(tmp_path):
    from piml_amd.data.data import RawData
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'x_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--seeds', '0:4', '--frames', '100',
                        '--out', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count('[simulate] gc (seed ') == 4 and 'mean +- std' in p.stdout
    for s in range(4):
        raw = RawData()
        raw.load_trajectory_data(out.replace('{seed}', str(s)))
        assert raw.num_pedestrians >= 20
