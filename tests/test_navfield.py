"""CPU: the floor field's numpy restatement (nav_ref.py) on an empty grid -- 1-Lipschitz, between the Euclidean and the
Manhattan distance, a fixed point --, the argument checks of piml_nav_relax, piml_nav_direction and
piml_scenario_step_mlapm_nav that return before any HIP call, the gfx950 build of the nav kernels without scratch, the Python
refusals of scenes a field cannot route, and the floor plan's JSON and command line."""
import ctypes
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref as REF
from conftest import REPO

f32 = np.float32


# ---- 1. the restatement ----

def test_restatement_on_an_empty_grid():
    gx = gy = 65
    blocked = np.zeros((gy, gx), np.uint8)
    goal = np.zeros((1, gy, gx), np.uint8)
    goal[0, 32, 32] = 1
    u, n = REF.solve(blocked, goal)
    assert n == 64                                               # the corner is 64 cells of Manhattan distance away
    again = REF.jacobi_step(u, blocked, goal)
    assert np.array_equal(again.view(np.uint32), u.view(np.uint32))           # a fixed point
    u = u[0].astype(np.float64)
    assert np.isfinite(u).all() and u[32, 32] == 0
    yy, xx = np.mgrid[:gy, :gx]
    assert (u >= np.hypot(xx - 32, yy - 32)).all() and (u <= np.abs(xx - 32) + np.abs(yy - 32)).all()
    assert np.abs(np.diff(u, axis=0)).max() <= 1.0 and np.abs(np.diff(u, axis=1)).max() <= 1.0     # 1-Lipschitz, exactly
    # u only decreases from step to step
    a = REF.start(goal)
    for _ in range(5):
        b = REF.jacobi_step(a, blocked, goal)
        assert (b <= a).all()
        a = b


def test_restatement_with_a_u_shaped_wall():
    blocked, goal = REF.u_shape_case()
    u, n = REF.solve(blocked, goal)
    assert 33 < n < 33 * 34                                      # round the wall: more than one launch of 8, well under gx gy
    assert np.isinf(u[:, 20, 30]).all()                          # the enclosed free cell
    assert u[1, 5, 8] == 0 and np.isinf(u[0, 5, 8])              # a goal on a blocked cell: free for its own gate only
    free = blocked == 0
    free[20, 30] = False
    assert np.isfinite(u[0][free]).all() and np.isfinite(u[1][free]).all()
    for g in range(2):                                           # 1-Lipschitz between free 4-neighbours
        v = np.where(free, u[g], np.nan).astype(np.float64)
        for d in (np.abs(np.diff(v, axis=0)), np.abs(np.diff(v, axis=1))):
            assert np.nanmax(d) <= 1.0
    # the field goes round the wall: inside the U, straight below the gate, is farther than the Manhattan distance
    assert u[0, 2, 17] > 6 + 9


def test_restated_lookup_takes_each_branch():
    blocked, goal = REF.u_shape_case()
    u, _ = REF.solve(blocked, goal)
    c = 0.25
    P = np.array([[17.5 * c, 20.5 * c], [17.5 * c, 8.6 * c], [9.2 * c, 10.5 * c], [-1.0, 1.0], [np.nan, 1.0], [30.5 * c, 20.5 * c],
                  [8.5 * c, 10.5 * c]], f32)
    dest = np.tile(np.array([[17.5 * c, 8.5 * c]], f32), (len(P), 1))
    e, b, k = REF.direction(u, 0.0, 0.0, c, 2.0, P, np.zeros(len(P), np.int32), dest)
    assert b.tolist() == [1, 0, 2, 0, 0, 0, 0]                   # open floor, near, beside the wall, outside, NaN, enclosed, blocked
    assert k[2] >= 0 and (k[b != 2] == -1).all()
    assert np.allclose(np.hypot(e[:4, 0], e[:4, 1]), 1.0) and e[0, 1] < -0.9           # down the U to the gate


# ---- 2. argument refusal without a GPU ----

def _fake_nav(**kw):
    """a descriptor that passes every check, over a buffer that is never read: every call below is refused or empty"""
    from piml_amd import _lib
    buf = (ctypes.c_float * 8)()
    g = _lib.NavGrid()
    g.u = ctypes.addressof(buf)
    g.G, g.gx, g.gy = 2, 4, 5
    g.x0, g.y0, g.cell, g.near = -1.0, 2.0, 0.25, 2.0
    for k, v in kw.items():
        setattr(g, k, v)
    g._keep = buf
    return g


BAD_NAVS = [dict(u=None), dict(G=0), dict(G=65), dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025), dict(gy=-3),
            dict(cell=0.0), dict(cell=-1.0), dict(cell=float('nan')), dict(cell=float('inf')), dict(x0=float('nan')),
            dict(x0=float('inf')), dict(y0=float('-inf')), dict(near=-0.5), dict(near=float('nan')), dict(near=float('inf'))]


def test_nav_relax_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    buf, other = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    a, b = ctypes.addressof(buf), ctypes.addressof(other)

    def call(blocked=a, goal=a, u_a=a, u_b=b, G=1, gx=2, gy=2, launches=0, changed=a):
        return L.piml_nav_relax(blocked, goal, u_a, u_b, G, gx, gy, launches, changed, None)
    assert call() == 0 and call(G=64, gx=1024, gy=1) == 0       # no launch: the baseline passes every check
    for kw in (dict(blocked=None), dict(goal=None), dict(u_a=None), dict(u_b=None), dict(u_b=a), dict(changed=None), dict(G=0),
               dict(G=65), dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025), dict(launches=-1)):
        assert call(**kw) == 1, kw


def test_nav_direction_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    a = ctypes.addressof(buf)
    good = _fake_nav()

    def call(rows=0, g=good, pos=a, gate=a, dest=a, out=a):
        return L.piml_nav_direction(pos, gate, dest, rows, None if g is None else ctypes.byref(g), out, None, None, None)
    assert call() == 0 and call(pos=None, gate=None, dest=None) == 0          # rows == 0: nothing to read
    assert call(rows=-1) == 1 and call(g=None) == 1 and call(out=None) == 1 and call(rows=3, out=None) == 1
    assert call(rows=3, pos=None) == 1 and call(rows=3, gate=None) == 1 and call(rows=3, dest=None) == 1
    for kw in BAD_NAVS:
        assert call(g=_fake_nav(**kw)) == 1 and call(rows=3, g=_fake_nav(**kw)) == 1, kw


def _fake_scene(**kw):
    """a GC descriptor that passes the frame checks, over buffers that are never read (every call below is refused)"""
    from piml_amd import _lib
    buf = (ctypes.c_float * 8)()
    s = _lib.Scenario()
    for name, kind in _lib.Scenario._fields_:
        if kind is ctypes.c_void_p:
            setattr(s, name, ctypes.addressof(buf))
    s.hist_width, s.F, s.D, s.E, s.P, s.R, s.capacity, s.T = 2, 7, 2, 2, 1, 2, 4, 3
    s.n_initial, s.route_max_iters, s.spawn_cap, s.dt = 1, 0, 0, 0.08
    for k, v in kw.items():
        setattr(s, k, v)
    s._keep = buf
    return s


def test_scenario_nav_entry_refuses_bad_arguments_without_gpu():
    """every call is refused: the one argument set that would pass (checked on the GPU) differs from each in one thing"""
    from piml_amd import _lib, ops_scenario
    from test_wallforce import BAD_GRIDS, _fake_grid
    L = _lib.lib()
    s, law, nav = _fake_scene(), ops_scenario.mlapm_law(), _fake_nav()
    seeds = (ctypes.c_uint64 * 1)(0)
    table = ctypes.addressof(nav._keep)
    ref = ctypes.byref

    def call(s_=s, r=None, members=1, seeds_=seeds, law_=law, table_=None, g=None, wall=None, wtable=None, nav_=nav, noise=None,
             offset=0):
        opt = lambda x: None if x is None else ref(x)
        return L.piml_scenario_step_mlapm_nav(opt(s_), opt(r), members, seeds_, opt(law_), table_, opt(g), opt(wall), wtable,
                                              opt(nav_), opt(noise), offset, None)
    # the frame checks
    assert call(s_=None) == 1 and call(s_=_lib.Scenario()) == 1 and call(members=0) == 1 and call(members=65536) == 1
    assert call(seeds_=None) == 1 and call(offset=-1) == 1
    bad_law = ops_scenario.mlapm_law()
    bad_law.tau = 0.0
    assert call(law_=bad_law) == 1 and call(law_=None) == 1 and call(table_=table) == 1       # exactly one of law / table
    # the field's own: a scene rule, a detour route, another number of gates, a bad grid
    for law_name in ('crosswalk', 'square', 'unit1', 'clip'):
        r = _lib.ScenarioRules()
        r.spawn_law, r.arrival_rule = _lib.SPAWN_LAWS[law_name], _lib.ARRIVAL_RULES['radius']
        assert call(r=r) == 1, law_name
    r = _lib.ScenarioRules()
    r.spawn_law = _lib.SPAWN_CLIP_GROUPS
    assert call(r=r) == 1
    assert call(s_=_fake_scene(route_max_iters=1)) == 1 and call(s_=_fake_scene(route_max_iters=16)) == 1
    assert call(nav_=_fake_nav(G=3)) == 1 and call(s_=_fake_scene(E=3)) == 1 and call(nav_=None) == 1
    for kw in BAD_NAVS:
        assert call(nav_=_fake_nav(**kw)) == 1, kw
    # the wall term's and the fluctuation term's
    wall = ops_scenario.wall_law(50.0, -5.0)
    assert call(wall=wall) == 1 and call(wtable=table) == 1                    # a wall law without a grid
    assert call(g=_fake_grid()) == 1 and call(g=_fake_grid(), wall=wall, wtable=table) == 1
    for kw in BAD_GRIDS[:6]:
        assert call(g=_fake_grid(**kw), wall=wall) == 1, kw
    noise = _lib.NoiseArgs()
    assert call(noise=noise) == 1                                # no state
    noise.state, noise.law.rho, noise.law.amp = table, 1.5, 1.0
    assert call(noise=noise) == 1                                # rho outside [0, 1)


def test_header_declares_and_lib_binds_the_entries():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    for name in ('piml_nav_relax', 'piml_nav_direction', 'piml_scenario_step_mlapm_nav'):
        assert re.search(r'\bint %s\s*\(' % name, text) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert 'typedef struct piml_nav_grid' in text
    assert [f for f, _ in _lib.NavGrid._fields_] == ['u', 'G', 'gx', 'gy', 'x0', 'y0', 'cell', 'near']
    assert ctypes.sizeof(_lib.NavGrid) == 40
    assert len(_lib.SIGNATURES['piml_nav_relax']) == 10 and len(_lib.SIGNATURES['piml_nav_direction']) == 9
    assert len(_lib.SIGNATURES['piml_scenario_step_mlapm_nav']) == 13
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols and structs were only added


# ---- 3. build ----

def test_nav_kernels_build_for_gfx950_without_scratch(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'nav.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'nav.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    report = re.findall(r'Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    names = [n for n, _ in report if n]
    scratch = [int(s) for _, s in report if s]
    assert len(names) == len(scratch), names
    assert any('nav_relax_kernel' in n for n in names) and any('nav_direction_kernel' in n for n in names), names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    lds = [int(x) for x in re.findall(r'LDS Size \[bytes/block\]: (\d+)', p.stderr)]
    assert max(lds) == 2 * 48 * 48 * 4 + 48 * 48                 # two staged planes and the fixed flags


def test_nav_kernels_do_not_spill():
    pytest.importorskip('msgpack')
    from piml_amd import _lib
    usage = _lib.kernel_resource_usage()
    for name in ('nav_relax_kernel', 'nav_direction_kernel'):
        assert name in usage, name
        assert usage[name]['vgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, (name, usage[name])
    for name in ('scenario_mlapm_nav_kernel<false, false>', 'scenario_mlapm_nav_kernel<false, true>',
                 'scenario_mlapm_nav_kernel<true, false>', 'scenario_mlapm_nav_kernel<true, true>'):
        assert name in usage, name
        assert usage[name]['vgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, (name, usage[name])


# ---- 4. Python checks ----

BASE = {'version': 'GC', 'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
PLAN = {'walls': [[[5.0, -1.0], [5.0, 4.5]], [[5.0, 5.5], [5.0, 11.0]]],
        'gates': [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]}


def test_scenes_the_field_cannot_route_are_refused():
    import torch
    from piml_amd import ops_scenario, scenarios
    from piml_amd.models import mlapm
    gc = scenarios.gc_scenario()
    ops_scenario.check_nav_scene(dataclasses.replace(gc, route_max_iters=0))
    with pytest.raises(ValueError, match='route_max_iters'):
        ops_scenario.check_nav_scene(gc)
    with pytest.raises(ValueError, match='grouped'):
        ops_scenario.check_nav_scene(dataclasses.replace(gc, route_max_iters=0, spawn_law='clip_groups'))
    for sc in (scenarios.crosswalk_scenario(), scenarios.four_directional_square_scenario(), scenarios.basic_unit1_scenario(),
               dataclasses.replace(gc, route_max_iters=0, spawn_law='clip')):
        with pytest.raises(ValueError, match='gates'):
            ops_scenario.check_nav_scene(sc)
    sim = mlapm.MLAPM(**BASE)
    with pytest.raises(ValueError, match='route_max_iters'):    # refused before any state is allocated
        sim.simulate_scenario(gc, 5, device='cpu', nav=True)
    with pytest.raises(ValueError, match='gates'):
        sim.simulate_ensemble(scenarios.crosswalk_scenario(), 5, [0, 1], device='cpu', nav=True)
    with pytest.raises(ValueError, match='route_max_iters'):
        mlapm.MLAPM.simulate_sweep(gc, 5, [BASE], [0, 1], device='cpu', nav=True)
    with pytest.raises(ValueError, match='route_max_iters'):
        mlapm.SweepRun(gc, 5, 1, [0], device='cpu', nav=True)
    # the operators have no CPU path
    from piml_amd import _lib
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_field(dataclasses.replace(gc, route_max_iters=0), device='cpu')
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_relax(torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(1, 3, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops_scenario.nav_relax(torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, dtype=torch.uint8))
    for bad in (dict(cell=0.0), dict(cell=float('nan')), dict(clearance=0.0), dict(near=-1.0)):
        with pytest.raises((ValueError, _lib.PimlHipError)):
            ops_scenario.nav_field(dataclasses.replace(gc, route_max_iters=0), device='cuda', **bad)


def test_grid_of_a_scene_on_the_host():
    from piml_amd import ops_scenario, scenarios
    sc = scenarios.floorplan_scenario(PLAN['walls'], PLAN['gates'])
    g = ops_scenario.nav_grid_host(sc, 0.25)
    pad = 0.8 + 0.25                                             # spawn_offset + cell around walls and gates
    assert (g.x0, g.y0) == (float(f32(0.0 - pad)), float(f32(-1.0 - pad))) and g.cell == 0.25
    assert g.gx == int(np.ceil((10.0 + 2 * pad) / 0.25)) and g.gy == int(np.ceil((12.0 + 2 * pad) / 0.25))
    assert g.centres.shape == (g.gy, g.gx, 2) and g.centres.dtype == f32
    assert g.centres[0, 0].tolist() == [float(f32(g.x0) + f32(0.125)), float(f32(g.y0) + f32(0.125))]
    assert g.goal.shape == (2, g.gy, g.gx) and g.goal.dtype == np.uint8
    ent = sc.entries.numpy()
    for e in range(2):                                           # exactly the cells that hold the gate's points
        cells = {(int(np.floor((q[0] - f32(g.x0)) / f32(0.25))), int(np.floor((q[1] - f32(g.y0)) / f32(0.25)))) for q in ent[e]}
        ys, xs = np.nonzero(g.goal[e])
        assert set(zip(xs.tolist(), ys.tolist())) == cells and len(cells) >= 10
    g = ops_scenario.nav_grid_host(sc, 0.5, bounds=(-1.0, -1.0, 11.0, 7.0))
    assert (g.gx, g.gy, g.x0, g.y0) == (24, 16, -1.0, -1.0)
    with pytest.warns(UserWarning, match='coarsened'):
        g = ops_scenario.nav_grid_host(sc, 0.25, bounds=(-1000.0, -1.0, 1000.0, 7.0))
    assert g.gx <= 1024 and g.gy <= 1024 and g.cell > 0.25
    with pytest.raises(ValueError, match='no point inside'):
        ops_scenario.nav_grid_host(sc, 0.25, bounds=(2.0, -1.0, 11.0, 7.0))
    for bad in (dict(cell=0.0), dict(cell=float('inf')), dict(bounds=(0.0, 0.0, 0.0, 5.0)), dict(bounds=(0.0, 0.0, float('nan'), 5.0))):
        with pytest.raises(ValueError):
            ops_scenario.nav_grid_host(sc, **{'cell': 0.25, **bad})


def test_floorplan_scenario_and_json(tmp_path):
    from piml_amd import scenarios
    sc = scenarios.floorplan_scenario(PLAN['walls'], PLAN['gates'], rate_per_s=2.0, n_initial=6, gate_points=20, time_unit=0.08,
                                      arrival_radius=0.7)
    assert 'floorplan' not in scenarios.SCENARIOS
    assert sc.spawn_law == 'gc' and sc.arrival_rule == 'gc' and sc.route_max_iters == 0 and sc.name == 'floorplan'
    assert tuple(sc.entries.shape) == (2, 20, 2) and tuple(sc.route_polyline.shape) == (2, 2)
    assert sc.rate_per_s == 2.0 and sc.n_initial == 6 and sc.arrival_radius == 0.7 and sc.num_waypoints == 2
    assert sc.entries[0, 0].tolist() == [0.0, 0.5] and sc.entries[1, -1].tolist() == [10.0, 3.0]
    obs = sc.obstacles.numpy()
    assert obs.shape == (2 * (int(np.ceil(5.5 / 0.05)) + 1), 2) and (obs[:, 0] == 5.0).all()
    assert not ((obs[:, 1] > 4.5) & (obs[:, 1] < 5.5)).any() and obs[:, 1].min() == -1.0 and obs[:, 1].max() == 11.0
    assert np.diff(np.sort(obs[:, 1])).max() <= 1.0 + 1e-6 and np.diff(obs[obs[:, 1] <= 4.5, 1]).max() <= 0.05 + 1e-6
    assert scenarios.floorplan_scenario([], PLAN['gates']).obstacles.shape == (0, 2)
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, rate_per_s=2.0, n_initial=6, gate_points=20, arrival_radius=0.7, name='two_rooms')))
    got = scenarios.load_floorplan(str(path))
    assert got.name == 'two_rooms' and got.route_max_iters == 0 and got.arrival_radius == 0.7
    assert np.array_equal(got.entries.numpy(), sc.entries.numpy()) and np.array_equal(got.obstacles.numpy(), obs)
    for bad in (dict(PLAN, gates=PLAN['gates'][:1]), dict(PLAN, gates=[[[0, 0], [1, 1], [2, 2]]] * 2), dict(PLAN, walls=[[[0, 0]]]),
                dict(PLAN, walls=[[[0, 0], [1, float('nan')]]]), dict(PLAN, route_max_iters=4), dict(PLAN, spawn_law='clip'),
                dict(PLAN, colour='red'), dict(PLAN, gate_points=0), dict(PLAN, wall_spacing=0.0), {'walls': []}, [1, 2]):
        path.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            scenarios.load_floorplan(str(path))
    with pytest.raises(ValueError):
        scenarios.floorplan_scenario(PLAN['walls'], PLAN['gates'], route_max_iters=3)


def test_command_line_round_trip(tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, n_initial=4)))
    own, _ = simulate.get_args(['--law', 'mlapm', '--scene-plan', str(path), '--nav'])
    assert own.nav and own.nav_cell == 0.25 and own.nav_clearance == 0.3 and own.plan.n_initial == 4
    assert own.plan.route_max_iters == 0 and tuple(own.plan.entries.shape) == (2, 100, 2)
    own, _ = simulate.get_args(['--law', 'mlapm', '--scenario', 'gc', '--nav', '--nav-cell', '0.125', '--nav-clearance', '0.4',
                                '--seeds', '0:2', '--obstacle-stats', str(tmp_path / 'o.json')])
    assert own.nav and own.nav_cell == 0.125 and own.nav_clearance == 0.4 and own.plan is None
    own, _ = simulate.get_args(['--law', 'mlapm', '--scene-plan', str(path)])
    assert not own.nav and own.plan is not None                  # a plan without the field runs (and walks into its walls)
    own, _ = simulate.get_args(['--law', 'mlapm'])
    assert not own.nav and own.plan is None and own.scene_plan is None
    clip = str(tmp_path / 'clip.npy')
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(dict(PLAN, gates=PLAN['gates'][:1])))
    for argv in (['--law', 'mlapm', '--scene-plan', str(path), '--scene-from', clip],
                 ['--law', 'mlapm', '--scene-plan', str(path), '--scenario', 'crosswalk'],
                 ['--law', 'pinnsf', '--scene-plan', str(path)], ['--scene-plan', str(path)],
                 ['--law', 'mlapm', '--scene-plan', str(bad)], ['--law', 'mlapm', '--scene-plan', str(tmp_path / 'none.json')],
                 ['--law', 'pinnsf', '--nav'], ['--nav'], ['--law', 'mlapm', '--scenario', 'crosswalk', '--nav'],
                 ['--law', 'mlapm', '--scene-from', clip, '--nav'], ['--law', 'mlapm', '--nav-cell', '0.5'],
                 ['--law', 'mlapm', '--nav-clearance', '0.5'], ['--law', 'mlapm', '--nav', '--nav-cell', '0'],
                 ['--law', 'mlapm', '--nav', '--nav-clearance', '-1']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)


def test_pinnsf_with_a_plan_names_what_is_missing(tmp_path, capsys):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(PLAN))
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'pinnsf', '--scene-plan', str(path)])
    assert 'floor field' in capsys.readouterr().err
