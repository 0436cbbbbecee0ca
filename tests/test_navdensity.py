"""CPU: the density-aware floor field's numpy restatement (navcost_ref.py) -- f == 1 is nav_ref bit for bit, the solve from
the cold start is monotone and bounded by the static field, a warm start does NOT reach the fixed point, and the two-room,
two-door plan sends its probes to the far door once the near one is queued --, the argument checks of piml_nav_density,
piml_nav_cost, piml_nav_relax_cost and piml_scenario_step_mlapm_navdyn that return before any HIP call, the Python and
command-line refusals, and the gfx950 build of navdensity.hip without scratch."""
import ctypes
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref
import navcost_ref as REF
from conftest import REPO
from test_navfield import BAD_NAVS, BASE, PLAN, _fake_nav, _fake_scene

f32 = np.float32
NAN, INF = float('nan'), float('inf')


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. the restatement ----

def test_unit_cost_is_the_static_field_bit_for_bit():
    for blocked, goal in (nav_ref.u_shape_case(), REF.two_door_case()[:2]):
        one = np.ones(blocked.shape, f32)
        u, v = nav_ref.start(goal), nav_ref.start(goal)
        for _ in range(12):                                      # step by step, not only at the fixed point
            u, v = nav_ref.jacobi_step(u, blocked, goal), REF.jacobi_step(v, blocked, goal, one)
            assert np.array_equal(bits(u), bits(v))
        us, ns = nav_ref.solve(blocked, goal)
        uc, nc = REF.solve(blocked, goal, one)
        assert nc == ns and np.array_equal(bits(us), bits(uc))
    assert ns == 58                                              # the two-room grid


def test_cold_start_is_monotone_and_bounded_by_the_static_field():
    blocked, goal = nav_ref.u_shape_case()
    f = np.random.default_rng(0).uniform(1, 4, blocked.shape).astype(f32)
    a = nav_ref.start(goal)
    for _ in range(20):
        b = REF.jacobi_step(a, blocked, goal, f)
        assert (b <= a).all()                                    # u only decreases: 'a batch changed nothing' is a fixed point
        a = b
    us, _ = nav_ref.solve(blocked, goal)
    u, n = REF.solve(blocked, goal, f)
    assert n == 84
    assert np.array_equal(bits(REF.jacobi_step(u, blocked, goal, f)), bits(u))
    fin = np.isfinite(us)
    assert np.array_equal(np.isfinite(u), fin)                   # the finite set is the static field's
    assert (us[fin] <= u[fin]).all() and (u[fin].astype(np.float64) <= float(f.max()) * us[fin].astype(np.float64)).all()


def test_a_warm_start_does_not_reach_the_fixed_point():
    """why every update restarts cold: min(cand, u) keeps the stale low values of the cheaper field"""
    blocked, goal = nav_ref.u_shape_case()
    f = np.random.default_rng(0).uniform(1, 4, blocked.shape).astype(f32)
    cold, n = REF.solve(blocked, goal, f)
    static, _ = nav_ref.solve(blocked, goal)
    warm = REF.steps(static, blocked, goal, f, 400)
    assert n == 84 and not np.array_equal(bits(warm), bits(cold))
    fin = np.isfinite(cold)
    assert (warm[fin] <= cold[fin]).all() and (warm[fin] < cold[fin]).any()     # too low, and it stays there
    assert np.array_equal(bits(REF.jacobi_step(warm, blocked, goal, f)), bits(warm))


def test_deposit_and_cost_restated():
    P = np.array([[[0.0, 0.0], [0.5, 0.0], [0.49999, 0.99], [-0.001, 0.2], [1.0, 0.2], [0.2, 1.5], [NAN, 0.1], [0.7, 0.7]]], f32)
    mask = np.array([[1, 1, 1, 1, 1, 1, 1, 0]], f32)
    c = REF.deposit(P, mask, 0.0, 0.0, 0.5, 2, 3)
    assert c.tolist() == [[[1, 1], [1, 0], [0, 0]]]              # x = 1.0 and y = 1.5 are the outer edges: outside
    s = REF.window_sum(np.arange(12).reshape(3, 4), 1)
    assert s[0, 0] == 0 + 1 + 4 + 5 and s[1, 1] == sum((0, 1, 2, 4, 5, 6, 8, 9, 10)) and s[2, 3] == 6 + 7 + 10 + 11
    assert REF.window_sum(np.ones((2, 3), np.int32), 8).tolist() == [[6] * 3] * 2          # a window larger than the grid
    cnt = np.array([[0, 9, 0], [0, 0, 0]], np.int32)
    f, rho = REF.cost(cnt, 1.0, 1, 2.0, 0.5, 8.0)
    assert rho[0, 0] == 1.0 and f[0, 0] == 2.0                   # 9 agents over 9 m^2; 1 + 2 (1 - 0.5)
    f, rho = REF.cost(cnt, 1.0, 0, 2.0, 9.0, 8.0)
    assert rho[0, 1] == 9.0 and (f == 1.0).all()                 # rho exactly at rho0: no rise
    f, _ = REF.cost(cnt, 1.0, 0, 2.0, 0.5, 8.0)
    assert f[0, 1] == 8.0 and f[0, 0] == 1.0                     # clipped at fmax
    assert (REF.cost(cnt, 1.0, 1, 0.0, 0.5, 8.0)[0] == 1.0).all()           # kd = 0


def test_two_doors_the_prototype_figures():
    blocked, goal, count = REF.two_door_case()
    assert count.sum() == 25
    want = {0.0: (58, [True] * 7), 2.0: (63, [False, False, False, False, False, True, False])}
    for kd, (steps, at_near) in want.items():
        f, rho = REF.cost(count, REF.TWO_DOOR_CELL, 1, kd, 0.5, 8.0)
        assert rho.max() == 4.0 and f.max() == (8.0 if kd else 1.0)
        u, n = REF.solve(blocked, goal, f)
        assert n == steps
        rows = [REF.descend(u[0], x, y, REF.TWO_DOOR_WALL) for x, y in REF.TWO_DOOR_PROBES]
        assert [r in REF.NEAR_DOOR for r in rows] == at_near, (kd, rows)
        assert all(r in REF.NEAR_DOOR + REF.FAR_DOOR for r in rows), (kd, rows)
    # the deposit of the queue's centres is the count plane
    c = REF.deposit(REF.two_door_positions()[None], np.ones((1, 25), f32), 0.0, 0.0, REF.TWO_DOOR_CELL, 40, 24)
    assert np.array_equal(c[0], count)


# ---- 2. the entries' refusals, without a device ----

def _bufs():
    buf, other = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    return buf, other, ctypes.addressof(buf), ctypes.addressof(other)


def test_nav_density_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(pos=a, mask=a, members=1, cap=4, x0=0.0, y0=0.0, cell=0.5, gx=2, gy=2, count=b):
        return L.piml_nav_density(pos, mask, members, cap, x0, y0, cell, gx, gy, count, None)
    for kw in (dict(pos=None), dict(mask=None), dict(count=None), dict(members=0), dict(members=65536), dict(cap=0), dict(cap=-1),
               dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025), dict(cell=0.0), dict(cell=-1.0), dict(cell=NAN),
               dict(cell=INF), dict(x0=NAN), dict(x0=INF), dict(y0=-INF), dict(y0=NAN)):
        assert call(**kw) == 1, kw


def test_nav_cost_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(count=a, members=1, gx=2, gy=2, cell=0.5, r=1, kd=2.0, rho0=0.5, fmax=8.0, cost=b):
        return L.piml_nav_cost(count, members, gx, gy, cell, r, kd, rho0, fmax, cost, None)
    for kw in (dict(count=None), dict(cost=None), dict(members=0), dict(members=65536), dict(gx=0), dict(gx=1025), dict(gy=0),
               dict(gy=1025), dict(cell=0.0), dict(cell=NAN), dict(cell=INF), dict(r=-1), dict(r=9), dict(kd=-0.5), dict(kd=NAN),
               dict(kd=INF), dict(rho0=-0.1), dict(rho0=NAN), dict(rho0=INF), dict(fmax=0.5), dict(fmax=NAN), dict(fmax=INF)):
        assert call(**kw) == 1, kw


def test_nav_relax_cost_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(blocked=a, goal=a, cost=a, u_a=a, u_b=b, members=1, G=1, gx=2, gy=2, launches=0, changed=a):
        return L.piml_nav_relax_cost(blocked, goal, cost, u_a, u_b, members, G, gx, gy, launches, changed, None)
    assert call() == 0 and call(members=1023, G=64, gx=1024, gy=1) == 0          # no launch: these pass every check
    for kw in (dict(blocked=None), dict(goal=None), dict(cost=None), dict(u_a=None), dict(u_b=None), dict(u_b=a),
               dict(changed=None), dict(members=0), dict(members=-2), dict(G=0), dict(G=65), dict(gx=0), dict(gx=1025), dict(gy=0),
               dict(gy=1025), dict(launches=-1), dict(members=1024, G=64),                  # 65536 planes
               dict(members=2048, G=1, gx=1024, gy=1024),                                   # 2^31 cells
               dict(members=33, G=64, gx=1024, gy=1024)):
        assert call(**kw) == 1, kw
    assert call(members=2047, G=1, gx=1024, gy=1024) == 0                                   # 2^31 - 2^20 cells


def test_scenario_navdyn_entry_refuses_bad_arguments_without_gpu():
    """every call is refused: piml_scenario_step_mlapm_nav's refusals and a negative stride"""
    from piml_amd import _lib, ops_scenario
    from test_wallforce import BAD_GRIDS, _fake_grid
    L = _lib.lib()
    s, law, nav = _fake_scene(), ops_scenario.mlapm_law(), _fake_nav()
    seeds = (ctypes.c_uint64 * 1)(0)
    table = ctypes.addressof(nav._keep)
    ref = ctypes.byref

    def call(s_=s, r=None, members=1, seeds_=seeds, law_=law, table_=None, g=None, wall=None, wtable=None, nav_=nav, stride=0,
             noise=None, offset=0):
        opt = lambda x: None if x is None else ref(x)
        return L.piml_scenario_step_mlapm_navdyn(opt(s_), opt(r), members, seeds_, opt(law_), table_, opt(g), opt(wall), wtable,
                                                 opt(nav_), stride, opt(noise), offset, None)
    assert call(stride=-1) == 1 and call(stride=-(2 ** 40)) == 1
    assert call(s_=None) == 1 and call(s_=_lib.Scenario()) == 1 and call(members=0) == 1 and call(members=65536) == 1
    assert call(seeds_=None) == 1 and call(offset=-1) == 1
    bad_law = ops_scenario.mlapm_law()
    bad_law.tau = 0.0
    assert call(law_=bad_law) == 1 and call(law_=None) == 1 and call(table_=table) == 1
    for law_name in ('crosswalk', 'square', 'unit1', 'clip'):
        r = _lib.ScenarioRules()
        r.spawn_law, r.arrival_rule = _lib.SPAWN_LAWS[law_name], _lib.ARRIVAL_RULES['radius']
        assert call(r=r) == 1, law_name
    r = _lib.ScenarioRules()
    r.spawn_law = _lib.SPAWN_CLIP_GROUPS
    assert call(r=r) == 1
    assert call(s_=_fake_scene(route_max_iters=1)) == 1
    assert call(nav_=_fake_nav(G=3)) == 1 and call(s_=_fake_scene(E=3)) == 1 and call(nav_=None) == 1
    for kw in BAD_NAVS:
        assert call(nav_=_fake_nav(**kw), stride=8) == 1, kw
    wall = ops_scenario.wall_law(50.0, -5.0)
    assert call(wall=wall) == 1 and call(wtable=table) == 1
    assert call(g=_fake_grid()) == 1 and call(g=_fake_grid(), wall=wall, wtable=table) == 1
    for kw in BAD_GRIDS[:6]:
        assert call(g=_fake_grid(**kw), wall=wall) == 1, kw
    noise = _lib.NoiseArgs()
    assert call(noise=noise) == 1
    noise.state, noise.law.rho, noise.law.amp = table, 1.5, 1.0
    assert call(noise=noise) == 1


def test_header_declares_and_lib_binds_the_entries():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    for name, n in (('piml_nav_density', 11), ('piml_nav_cost', 11), ('piml_nav_relax_cost', 12),
                    ('piml_scenario_step_mlapm_navdyn', 14)):
        assert re.search(r'\bint %s\s*\(' % name, text) and hasattr(_lib.lib(), name), name
        assert len(_lib.SIGNATURES[name]) == n, name
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols were only added


# ---- 3. build ----

def test_navdensity_kernels_build_for_gfx950_without_scratch(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'navdensity.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'navdensity.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    report = re.findall(r'Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    names = [n for n, _ in report if n]
    scratch = [int(s) for _, s in report if s]
    assert len(names) == len(scratch) == 3, names
    for k in ('nav_density_kernel', 'nav_cost_kernel', 'nav_relax_cost_kernel'):
        assert any(k in n for n in names), names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    lds = [int(x) for x in re.findall(r'LDS Size \[bytes/block\]: (\d+)', p.stderr)]
    assert max(lds) == 3 * 48 * 48 * 4 + 48 * 48                 # two staged planes, the cost plane and the fixed flags


# ---- 4. Python checks ----

def test_density_law_is_checked():
    from piml_amd import ops_scenario
    law = ops_scenario.nav_density_law(2.0)
    assert (law.kd, law.rho0, law.radius, law.fmax, law.every) == (2.0, 0.5, 0.75, 8.0, 8)
    assert law.radius_cells(0.25) == 3 and law.radius_cells(0.5) == 2 and ops_scenario.nav_density_law(0, radius=0).radius_cells(0.25) == 0
    assert ops_scenario.nav_density_law(1.0, radius=2.0).radius_cells(0.25) == 8
    with pytest.raises(ValueError, match='more than 8'):
        ops_scenario.nav_density_law(1.0, radius=2.2).radius_cells(0.25)
    with pytest.raises(TypeError):
        ops_scenario.nav_density_law()                           # kd has no default
    for bad in (dict(kd=-1.0), dict(kd=NAN), dict(kd=INF), dict(rho0=-0.1), dict(rho0=NAN), dict(radius=-1.0), dict(radius=INF),
                dict(fmax=0.99), dict(fmax=NAN), dict(fmax=INF), dict(every=0), dict(every=-8), dict(every=2.5), dict(every=True)):
        with pytest.raises(ValueError):
            ops_scenario.nav_density_law(**{'kd': 2.0, **bad})


def test_runs_a_density_term_cannot_join_are_refused():
    import torch
    from piml_amd import _lib, ops_scenario, scenarios
    from piml_amd.models import mlapm
    from piml_amd.models.simulators import BaseSimulator
    gc = dataclasses.replace(scenarios.gc_scenario(), route_max_iters=0)
    law = ops_scenario.nav_density_law(2.0)
    sim = mlapm.MLAPM(**BASE)
    # without a field, with the any-angle table, or something that is no law: before any state is allocated
    with pytest.raises(ValueError, match='needs nav'):
        sim.simulate_scenario(gc, 5, device='cpu', nav_density=law)
    with pytest.raises(ValueError, match='needs nav'):
        sim.simulate_ensemble(gc, 5, [0, 1], device='cpu', nav=False, nav_density=law)
    with pytest.raises(ValueError, match='any-angle'):
        sim.simulate_scenario(gc, 5, device='cpu', nav='sight', nav_density=law)
    with pytest.raises(ValueError, match='any-angle'):
        mlapm.MLAPM.simulate_sweep(gc, 5, [BASE], [0, 1], device='cpu', nav='sight', nav_density=law)
    with pytest.raises(ValueError, match='needs nav'):
        mlapm.SweepRun(gc, 5, 1, [0], device='cpu', nav_density=law)
    with pytest.raises(TypeError, match='nav_density_law'):
        sim.simulate_scenario(gc, 5, device='cpu', nav=True, nav_density=2.0)
    # the scenes a field cannot route stay refused (check_nav_scene): grouped, clip and synthetic scenes
    with pytest.raises(ValueError, match='grouped'):
        sim.simulate_scenario(dataclasses.replace(gc, spawn_law='clip_groups'), 5, device='cpu', nav=True, nav_density=law)
    with pytest.raises(ValueError, match='gates'):
        sim.simulate_scenario(dataclasses.replace(gc, spawn_law='clip'), 5, device='cpu', nav=True, nav_density=law)
    with pytest.raises(ValueError, match='gates'):
        sim.simulate_ensemble(scenarios.crosswalk_scenario(), 5, [0, 1], device='cpu', nav=True, nav_density=law)
    # the network-driven frame: not built
    for name in ('simulate_scenario', 'simulate_ensemble'):
        with pytest.raises(NotImplementedError, match='not built'):
            getattr(BaseSimulator, name)(None, gc, 5, [0], nav=True, nav_density=law)
    # the operators have no CPU path and check their shapes
    with pytest.raises(TypeError):
        ops_scenario.nav_density(torch.zeros(4, 2), torch.zeros(4), None)
    with pytest.raises(TypeError):
        ops_scenario.nav_field_update(None, None, law)
    with pytest.raises(TypeError):
        ops_scenario.NavFieldDynamic(None, 2)
    z8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_relax_cost(z8(3, 3), z8(1, 3, 3), torch.ones(1, 3, 3))
    with pytest.raises(ValueError):
        ops_scenario.nav_relax_cost(z8(3, 3), z8(1, 3, 4), torch.ones(1, 3, 3))


def test_command_line(tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, n_initial=4)))
    own, _ = simulate.get_args(['--law', 'mlapm', '--scene-plan', str(path), '--nav', '--nav-density', '2'])
    law = own.density_law
    assert (law.kd, law.rho0, law.radius, law.fmax, law.every) == (2.0, 0.5, 0.75, 8.0, 8)
    own, _ = simulate.get_args(['--law', 'mlapm', '--scenario', 'gc', '--nav', '--nav-density', '1.5', '--nav-rho0', '1',
                                '--nav-density-radius', '0.5', '--nav-fmax', '4', '--nav-every', '32', '--seeds', '0:2',
                                '--line-stats', str(tmp_path / 'l.json'), '--lines', '0,2,30,2'])
    law = own.density_law
    assert (law.kd, law.rho0, law.radius, law.fmax, law.every) == (1.5, 1.0, 0.5, 4.0, 32)
    own, _ = simulate.get_args(['--law', 'mlapm', '--scene-plan', str(path), '--nav'])
    assert own.density_law is None
    head = ['--law', 'mlapm', '--scene-plan', str(path)]
    for argv in (head + ['--nav', '--nav-sight', '--nav-density', '2'], head + ['--route', 'sight', '--nav-density', '2'],
                 ['--checkpoint', 'm.pt', '--scene-plan', str(path), '--route', 'field', '--nav-density', '2'],
                 ['--law', 'pinnsf', '--scene-plan', str(path), '--route', 'field', '--nav-density', '2'],
                 head + ['--nav-density', '2'], head + ['--nav', '--nav-density', '-1'], head + ['--nav', '--nav-density', 'nan'],
                 head + ['--nav', '--nav-density', '2', '--nav-fmax', '0.5'], head + ['--nav', '--nav-density', '2', '--nav-every', '0'],
                 head + ['--nav', '--nav-density', '2', '--nav-rho0', '-1'],
                 head + ['--nav', '--nav-density', '2', '--nav-density-radius', '3'],        # 12 cells of 0.25
                 head + ['--nav', '--nav-rho0', '1'], head + ['--nav', '--nav-every', '8'], head + ['--nav', '--nav-fmax', '4'],
                 head + ['--nav', '--nav-density-radius', '1']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)
