"""CPU: the wall term's static cell grid (ops_scenario.wall_grid_host) -- its 3 x 3 neighbourhood query against the brute-force
restatement (wallforce_ref.py) on adversarial agents, its construction --, the argument checks of piml_wall_force and
piml_scenario_step_mlapm_walls that return before any HIP call, the gfx950 build of the wall kernels without scratch, and the
Python plumbing of Aw / Bw / wall_cutoff through MLAPM, simulate, the sweep and the statistics fit."""
import ctypes
import json
import math
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import wallforce_ref as REF
from conftest import REPO

f32 = np.float32


# ---- 1. exactness of the 3 x 3 neighbourhood ----

def query_3x3(g, P):
    """the kernel's search in numpy: the agent's cell by the grid's float32 formula, clamped to [-1, gx] x [-1, gy] as a
    float, three row-runs of the sorted list, the minimum of the key, the cutoff predicate"""
    P = np.asarray(P, f32)
    n = P.shape[0]
    index, dist2 = np.full(n, -1, np.int32), np.full(n, np.inf, f32)
    if g.n_points == 0:
        return index, dist2
    cell, c2 = f32(g.cell), f32(g.cutoff) * f32(g.cutoff)
    with np.errstate(invalid='ignore', over='ignore'):
        cx = np.clip(np.floor((P[:, 0] - f32(g.x0)) / cell), -1, g.gx)
        cy = np.clip(np.floor((P[:, 1] - f32(g.y0)) / cell), -1, g.gy)
    Q, cs = g.points, g.cell_start
    for i in range(n):
        if np.isnan(P[i]).any():
            continue
        x, y = int(cx[i]), int(cy[i])
        lo, hi = max(x - 1, 0), min(x + 1, g.gx - 1)
        if lo > hi:
            continue
        runs = [np.arange(cs[r * g.gx + lo], cs[r * g.gx + hi + 1]) for r in range(max(y - 1, 0), min(y + 1, g.gy - 1) + 1)]
        j = np.concatenate(runs) if runs else np.zeros(0, np.int64)
        if j.size == 0:
            continue
        ex, ey = Q[j, 0] - P[i, 0], Q[j, 1] - P[i, 1]
        d2 = ex * ex + ey * ey
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
        k = key.min()
        best = np.array([k >> np.uint64(32)], np.uint64).astype(np.uint32).view(f32)[0]
        if best < c2:
            index[i], dist2[i] = int(k & np.uint64(0xFFFFFFFF)), best
    return index, dist2


def ulps(x, k):
    """x moved by k float32 ulps (k may be negative), elementwise"""
    x = np.asarray(x, f32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def adversarial_agents(g, rng, n_random, n_edge, n_ring):
    """agents over the grid g: uniform over the box grown by three cutoffs (outside it by less and by more than the cutoff),
    within a few ulps of cell edges, and at distance cutoff (1 +- 2^-20) from a point"""
    cut, cell = g.cutoff, f32(g.cell)
    lo = np.array([g.x0, g.y0]) - 3 * cut
    hi = np.array([g.x0 + g.gx * g.cell, g.y0 + g.gy * g.cell]) + 3 * cut
    out = [rng.uniform(lo, hi, (n_random, 2)).astype(f32)]
    # cell edges: x0 + k cell as the float32 product and sum the formula inverts, moved by -3 .. 3 ulps, per axis
    kx, ky = rng.integers(-1, g.gx + 2, n_edge), rng.integers(-1, g.gy + 2, n_edge)
    ex = f32(g.x0) + kx.astype(f32) * cell
    ey = f32(g.y0) + ky.astype(f32) * cell
    other = rng.uniform(lo, hi, (n_edge, 2)).astype(f32)
    for k in (-3, -1, 0, 1, 3):
        sel = slice((k + 3) * n_edge // 7, (k + 4) * n_edge // 7)
        out.append(np.stack([ulps(ex[sel], k), other[sel, 1]], 1))
        out.append(np.stack([other[sel, 0], ulps(ey[sel], k)], 1))
        out.append(np.stack([ulps(ex[sel], k), ulps(ey[sel], -k)], 1))
    # rings: cutoff (1 +- 2^-20) away from a point, any direction (and along the axes, where the per-axis margin is tight)
    q = g.points[rng.integers(0, g.n_points, n_ring)].astype(np.float64)
    th = rng.uniform(0, 2 * np.pi, n_ring)
    th[::4] = np.round(th[::4] / (np.pi / 2)) * (np.pi / 2)
    r = cut * (1 + rng.choice([-1.0, 1.0], n_ring) * 2.0 ** -20)
    out.append((q + r[:, None] * np.stack([np.cos(th), np.sin(th)], 1)).astype(f32))
    return np.concatenate(out)


def scene_points(name, rng):
    from piml_amd import scenarios
    if name == 'gc':
        return scenarios.gc_scenario().obstacles.numpy()
    if name == 'square':
        return scenarios.four_directional_square_scenario().obstacles.numpy()
    return rng.uniform([0, 0], [40, 25], (3000, 2)).astype(f32)          # dense: hundreds of points per neighbourhood


@pytest.mark.parametrize('name,cutoff,offset', [('gc', 2.0, 0.0), ('gc', 2.0, 1000.0), ('gc', 0.7, -1000.0),
                                                ('random', 2.0, 0.0), ('random', 1.3, 1000.0), ('square', 2.0, -1000.0)])
def test_3x3_neighbourhood_is_exact(name, cutoff, offset):
    """the selection of the 3 x 3 query is identical to the brute-force one for every agent (index, d2, felt or not); if
    this fails the margin 1 + 2^-5 is wrong, not the test"""
    from piml_amd import ops_scenario
    rng = np.random.default_rng([len(name), int(cutoff * 10), int(offset) + 2000])
    obs = (scene_points(name, np.random.default_rng(5)) + f32(offset)).astype(f32)
    g = ops_scenario.wall_grid_host(obs, cutoff)
    assert g.cell >= f32(cutoff) * REF.MARGIN and g.gx <= 1024 and g.gy <= 1024
    P = adversarial_agents(g, rng, 1500, 1400, 1000)
    P[::97] = np.nan
    assert P.shape[0] >= 5000                                    # x 6 cases: more than 20 000 agents
    pts, order = REF.sorted_points(obs, cutoff)
    assert np.array_equal(pts, g.points) and np.array_equal(order, g.order)
    want_i, want_d = REF.select(P, pts, cutoff)
    got_i, got_d = query_3x3(g, P)
    assert np.array_equal(got_i, want_i), np.flatnonzero(got_i != want_i)[:10]
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    felt = want_i >= 0
    assert 0.05 < felt.mean() < 0.99                             # both outcomes are exercised
    ring = P[-1000:]
    assert (want_i[-1000:] >= 0).any() and (want_i[-1000:] < 0).any(), ring[:2]


# ---- 2. grid construction ----

def test_grid_drops_invalid_points_and_sorts_stably():
    from piml_amd import ops_scenario
    rng = np.random.default_rng(2)
    obs = rng.uniform(0, 9, (400, 2)).astype(f32)
    obs[::7, 0] = np.nan
    obs[3::11, 1] = np.inf
    obs[5::13] = -np.inf
    g = ops_scenario.wall_grid_host(obs, 1.0)
    valid = np.flatnonzero(np.isfinite(obs).all(1))
    assert g.n_points == valid.size and sorted(g.order.tolist()) == valid.tolist()
    assert np.array_equal(g.points, obs[g.order])
    assert g.cell_start.dtype == np.int32 and g.cell_start.shape == (g.gx * g.gy + 1,)
    assert g.cell_start[0] == 0 and g.cell_start[-1] == g.n_points and (np.diff(g.cell_start) >= 0).all()
    cell = f32(g.cell)
    for c in range(g.gx * g.gy):
        a, b = g.cell_start[c], g.cell_start[c + 1]
        q = g.points[a:b]
        assert (np.floor((q[:, 0] - f32(g.x0)) / cell) == c % g.gx).all() and (np.floor((q[:, 1] - f32(g.y0)) / cell) == c // g.gx).all()
        assert (np.diff(g.order[a:b]) > 0).all()                 # list order is kept inside a cell
    assert (g.x0, g.y0) == tuple(float(v) for v in obs[valid].min(0))
    assert g.cell == float(f32(1.0) * REF.MARGIN) and g.cutoff == 1.0


def test_grid_small_and_degenerate_sets():
    from piml_amd import ops_scenario
    g = ops_scenario.wall_grid_host(np.zeros((0, 2), f32), 2.0)
    assert g.n_points == 0 and g.gx == g.gy == 1 and g.cell_start.tolist() == [0, 0]
    g = ops_scenario.wall_grid_host(np.full((3, 2), np.nan, f32), 2.0)
    assert g.n_points == 0
    g = ops_scenario.wall_grid_host([[3.5, -2.0]], 2.0)
    assert g.n_points == 1 and g.gx == g.gy == 1 and g.cell_start.tolist() == [0, 1] and (g.x0, g.y0) == (3.5, -2.0)
    i, d = query_3x3(g, np.array([[3.5, -2.0], [4.5, -2.0], [5.5, -2.0], [3.5, -4.0]], f32))
    assert i.tolist() == [0, 0, -1, -1] and d[:2].tolist() == [0.0, 1.0]       # d2 == c2 is not felt
    same = np.tile(np.array([[1.0, 1.0]], f32), (70, 1)) + np.linspace(0, 0.5, 70, dtype=f32)[:, None]
    g = ops_scenario.wall_grid_host(same, 2.0)                   # all points in one cell
    assert g.gx == g.gy == 1 and g.cell_start.tolist() == [0, 70] and g.order.tolist() == list(range(70))
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ops_scenario.wall_grid_host(same, bad)


def test_grid_is_coarsened_past_1024_cells_per_axis():
    from piml_amd import ops_scenario
    rng = np.random.default_rng(3)
    obs = np.concatenate([rng.uniform([0, 0], [5000, 30], (500, 2)), [[0, 0], [5000, 30]]]).astype(f32)
    with pytest.warns(UserWarning, match='coarsened'):
        g = ops_scenario.wall_grid_host(obs, 2.0)
    assert g.gx <= 1024 and g.gy <= 1024 and g.cell > 2.0 * float(REF.MARGIN)
    P = adversarial_agents(g, rng, 300, 70, 200)
    pts, _ = REF.sorted_points(obs, 2.0, cell=g.cell)
    assert np.array_equal(pts, g.points)
    want_i, want_d = REF.select(P, pts, 2.0)
    got_i, got_d = query_3x3(g, P)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ops_scenario.wall_grid_host(obs[:, ::-1] * f32(0.4), 2.0)           # 2000 m: 970 cells, no warning


# ---- 3. argument refusal without a GPU ----

def _fake_grid(**kw):
    """a descriptor that passes every check, over buffers that are never read: every call below is refused or empty"""
    from piml_amd import _lib
    buf = (ctypes.c_float * 8)()
    g = _lib.WallGrid()
    g.points = g.cell_start = ctypes.addressof(buf)
    g.n_points, g.gx, g.gy = 3, 4, 5
    g.x0, g.y0, g.cutoff = -1.0, 2.0, 2.0
    g.cell = float(f32(2.0) * REF.MARGIN)
    for k, v in kw.items():
        setattr(g, k, v)
    g._keep = buf
    return g


BAD_GRIDS = [dict(n_points=-1), dict(points=None), dict(cell_start=None), dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025),
             dict(gy=-3), dict(cell=float('nan')), dict(cell=float('inf')), dict(cell=0.0), dict(cell=-2.5),
             dict(cutoff=float('nan')), dict(cutoff=float('inf')), dict(cutoff=0.0), dict(cutoff=-2.0),
             dict(cell=2.0), dict(cell=float(np.nextafter(f32(2.0) * REF.MARGIN, f32(0)))), dict(x0=float('inf')),
             dict(x0=float('nan')), dict(y0=float('-inf')), dict(y0=float('nan'))]
BAD_LAWS = [(-1.0, -5.0), (-0.001, 0.0), (50.0, 0.001), (50.0, 5.0), (float('nan'), -5.0), (float('inf'), -5.0),
            (50.0, float('nan')), (50.0, float('-inf'))]


def test_wall_force_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    out = ctypes.addressof(buf)
    good = _fake_grid()
    call = lambda rows, g, A, B, force=out, pos=out: L.piml_wall_force(pos, rows, None if g is None else ctypes.byref(g), A, B,
                                                                       force, None, None, None)
    assert call(0, good, 50.0, -5.0) == 0                        # empty problems succeed: the baseline passes every check
    assert call(0, good, 0.0, 0.0) == 0
    assert call(7, _fake_grid(n_points=0, points=None, cell_start=None), 50.0, -5.0) == 0
    assert call(0, _fake_grid(gx=1024, gy=1), 50.0, -5.0) == 0
    assert call(-1, good, 50.0, -5.0) == 1
    assert call(0, None, 50.0, -5.0) == 1 and call(4, None, 50.0, -5.0) == 1
    assert call(0, good, 50.0, -5.0, force=None) == 1 and call(4, good, 50.0, -5.0, force=None) == 1
    assert call(4, good, 50.0, -5.0, pos=None) == 1
    for kw in BAD_GRIDS:
        assert call(0, _fake_grid(**kw), 50.0, -5.0) == 1, kw
        assert call(4, _fake_grid(**kw), 50.0, -5.0) == 1, kw
    for A, B in BAD_LAWS:
        assert call(0, good, A, B) == 1 and call(4, good, A, B) == 1, (A, B)


def _fake_scene():
    """a GC descriptor that passes the frame checks, over buffers that are never read (every call below is refused)"""
    from piml_amd import _lib
    buf = (ctypes.c_float * 8)()
    s = _lib.Scenario()
    for name, kind in _lib.Scenario._fields_:
        if kind is ctypes.c_void_p:
            setattr(s, name, ctypes.addressof(buf))
    s.hist_width, s.F, s.D, s.E, s.P, s.R, s.capacity, s.T = 2, 7, 2, 2, 1, 2, 4, 3
    s.n_initial, s.route_max_iters, s.spawn_cap, s.dt = 1, 4, 0, 0.08
    s._keep = buf
    return s


def test_scenario_walls_entry_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    s, law, wall, good = _fake_scene(), ops_scenario.mlapm_law(), ops_scenario.wall_law(50.0, -5.0), _fake_grid()
    seeds = (ctypes.c_uint64 * 1)(0)
    table = ctypes.addressof(good._keep)
    ref = ctypes.byref

    def call(s_=s, members=1, seeds_=seeds, law_=law, table_=None, g=good, wall_=wall, wtable=None, offset=0):
        return L.piml_scenario_step_mlapm_walls(None if s_ is None else ref(s_), None, members, seeds_,
                                                None if law_ is None else ref(law_), table_,
                                                None if g is None else ref(g), None if wall_ is None else ref(wall_), wtable,
                                                offset, None)
    # the frame checks of piml_scenario_step_mlapm / _laws
    assert call(s_=None) == 1 and call(s_=_lib.Scenario()) == 1 and call(members=0) == 1 and call(members=65536) == 1
    assert call(seeds_=None) == 1 and call(offset=-1) == 1
    bad_law = ops_scenario.mlapm_law()
    bad_law.tau = 0.0
    assert call(law_=bad_law) == 1
    # exactly one of each pair
    assert call(law_=None) == 1 and call(table_=table) == 1
    assert call(wall_=None) == 1 and call(wtable=table) == 1
    assert call(law_=None, table_=table, wall_=None) == 1
    # the grid checks and the by-value wall law's
    assert call(g=None) == 1
    for kw in BAD_GRIDS:
        assert call(g=_fake_grid(**kw)) == 1, kw
        assert call(g=_fake_grid(**kw), law_=None, table_=table) == 1, kw
    for A, B in BAD_LAWS:
        w = _lib.WallLaw()
        w.A, w.B = A, B
        assert call(wall_=w) == 1, (A, B)


def test_python_checks_of_the_wall_operators():
    import torch
    from piml_amd import _lib, ops_scenario
    for A, B in BAD_LAWS:
        with pytest.raises(ValueError):
            ops_scenario.wall_law(A, B)
        with pytest.raises(ValueError):
            ops_scenario.wall_law_table([(50.0, -5.0), (A, B)], device='cpu')
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.wall_grid(np.zeros((4, 2), f32), 2.0, device='cpu')
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.wall_law_table([(50.0, -5.0)], device='cpu')
    with pytest.raises(ValueError):
        ops_scenario.wall_law_table([])
    out = torch.zeros(2, 2)
    assert ops_scenario.wall_law_table([(50.0, -5.0), (0.0, 0.0)], out=out) is out and out.tolist() == [[50.0, -5.0], [0.0, 0.0]]
    with pytest.raises(ValueError):
        ops_scenario.wall_law_table([(50.0, -5.0)], out=out)
    h = ops_scenario.wall_grid_host(np.zeros((4, 2), f32), 2.0)
    grid = type('G', (), dict(cell_start=torch.zeros(2, dtype=torch.int32), n_points=4, desc=ops_scenario.wall_grid_desc(h, None, None)))
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.wall_force(torch.zeros(3, 2), grid, 50.0, -5.0)


def test_header_declares_and_lib_binds_the_entries():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint piml_wall_force\s*\(', text) and re.search(r'\bint piml_scenario_step_mlapm_walls\s*\(', text)
    assert 'typedef struct piml_wall_grid' in text and 'typedef struct piml_wall_law' in text
    assert [f for f, _ in _lib.WallGrid._fields_] == ['points', 'cell_start', 'n_points', 'gx', 'gy', 'x0', 'y0', 'cell', 'cutoff']
    assert [f for f, _ in _lib.WallLaw._fields_] == ['A', 'B'] and ctypes.sizeof(_lib.WallLaw) == 8
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols and structs were only added


# ---- 4. build ----

def test_wall_kernels_build_for_gfx950_without_scratch(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'walls.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'walls.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    report = re.findall(r'Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    names = [n for n, _ in report if n]
    scratch = [int(s) for _, s in report if s]
    assert len(names) == len(scratch) and any('wall_force_kernel' in n for n in names), names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))


def test_wall_kernels_do_not_spill():
    pytest.importorskip('msgpack')
    from piml_amd import _lib
    usage = _lib.kernel_resource_usage()
    for name in ('wall_force_kernel', 'scenario_mlapm_walls_kernel<false>', 'scenario_mlapm_walls_kernel<true>'):
        assert name in usage, name
        assert usage[name]['vgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, (name, usage[name])


# ---- 5. Python plumbing ----

BASE = {'version': 'GC', 'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}


def test_mlapm_accepts_the_wall_constants():
    from piml_amd.models import mlapm
    assert mlapm.wall_args(BASE) is None
    assert mlapm.wall_args({**BASE, 'Aw': 50, 'Bw': -5}) == (50.0, -5.0, 2.0)
    assert mlapm.wall_args({**BASE, 'Aw': 0, 'Bw': 0, 'wall_cutoff': 1.5}) == (0.0, 0.0, 1.5)
    mlapm.MLAPM(**BASE, Aw=50.0, Bw=-5.0, wall_cutoff=3.0)
    for bad in (dict(Aw=50.0), dict(Bw=-5.0), dict(wall_cutoff=2.0), dict(Aw=-1.0, Bw=-5.0), dict(Aw=50.0, Bw=0.1),
                dict(Aw=float('nan'), Bw=-5.0), dict(Aw=50.0, Bw=-5.0, wall_cutoff=0.0),
                dict(Aw=50.0, Bw=-5.0, wall_cutoff=float('inf'))):
        with pytest.raises(ValueError):
            mlapm.MLAPM(**BASE, **bad)
    assert mlapm.SWEEP_KEYS[-2:] == ('Aw', 'Bw') and 'wall_cutoff' not in mlapm.SWEEP_KEYS


def test_wall_term_needs_a_scene_with_obstacles():
    from piml_amd import scenarios
    from piml_amd.models import mlapm
    with pytest.raises(ValueError, match='no obstacles'):
        mlapm.check_scene_walls(scenarios.crosswalk_scenario())
    mlapm.check_scene_walls(scenarios.four_directional_square_scenario())
    sim = mlapm.MLAPM(**BASE, Aw=50.0, Bw=-5.0)
    with pytest.raises(ValueError, match='no obstacles'):       # refused before any state is allocated
        sim.simulate_scenario(scenarios.crosswalk_scenario(), 5, device='cpu')
    with pytest.raises(ValueError, match='no obstacles'):
        sim.simulate_ensemble(scenarios.crosswalk_scenario(), 5, [0, 1], device='cpu')


def test_sweep_laws_reject_mixed_candidates():
    from piml_amd.models import mlapm
    walled = {**BASE, 'Aw': 50.0, 'Bw': -5.0}
    assert len(mlapm.sweep_laws([walled, {**walled, 'Aw': 20.0}])) == 2
    assert mlapm.sweep_walls([walled, {**walled, 'Aw': 20.0, 'Bw': -1.0}]) == [(50.0, -5.0), (20.0, -1.0)]
    assert mlapm.sweep_walls([BASE, BASE]) is None
    for mixed in ([walled, BASE], [BASE, walled, walled], [{**BASE, 'Bw': -5.0}], [{**BASE, 'Aw': 5.0}],
                  [{**walled, 'wall_cutoff': 2.0}], [{**walled, 'Bw': 1.0}]):
        with pytest.raises(ValueError):
            mlapm.sweep_laws(mixed)


def test_params_json_and_cli_round_trip(tmp_path):
    from piml_amd import calibrate, simulate
    assert calibrate.WALL_PARAM_NAMES == ('Aw', 'Bw') and calibrate.PARAM_NAMES == ('tau', 'A', 'B', 'C', 'D', 'theta')
    walled = {**BASE, 'Aw': 50.0, 'Bw': -5.0, 'wall_cutoff': 1.5}
    path = tmp_path / 'walled.json'
    path.write_text(json.dumps(walled))
    assert simulate.load_mlapm_params(str(path)) == walled
    own, _ = simulate.get_args(['--law', 'mlapm', '--params', str(path), '--obstacle-stats', str(tmp_path / 'w.json')])
    assert own.mlapm == walled
    own, _ = simulate.get_args(['--law', 'mlapm'])
    assert 'Aw' not in own.mlapm and 'Bw' not in own.mlapm and 'wall_cutoff' not in own.mlapm       # no default wall term
    other = tmp_path / 'other.json'
    other.write_text(json.dumps({**walled, 'Aw': 20.0}))
    own, _ = simulate.get_args(['--law', 'mlapm', '--params-sweep', str(path), str(other), '--seeds', '0:2', '--stats',
                                str(tmp_path / 's.json')])
    assert own.wall_cutoff == 1.5 and [a['Aw'] for a in own.mlapm_sweep] == [50.0, 20.0]
    assert all('wall_cutoff' not in a for a in own.mlapm_sweep)
    plain = tmp_path / 'plain.json'
    plain.write_text(json.dumps(BASE))
    far = tmp_path / 'far.json'
    far.write_text(json.dumps({**walled, 'wall_cutoff': 3.0}))
    for files in ((path, plain), (path, far)):                   # mixed candidates; two cutoffs
        with pytest.raises(SystemExit):
            simulate.get_args(['--law', 'mlapm', '--params-sweep', *map(str, files), '--seeds', '0:2', '--stats', 'x.json'])
    for bad in ({**BASE, 'Aw': 50.0}, {**BASE, 'Bw': -5.0}, {**BASE, 'wall_cutoff': 2.0}, {**walled, 'Aw': 'big'},
                {**walled, 'Aw': -1.0}, {**walled, 'Bw': 0.5}, {**walled, 'wall_cutoff': 0.0}, {**walled, 'Cw': 1.0},
                {**walled, 'Aw': True}):
        badp = tmp_path / 'bad.json'
        badp.write_text(json.dumps(bad))
        with pytest.raises(SystemExit):
            simulate.get_args(['--law', 'mlapm', '--params', str(badp)])


def test_calibrate_cli_parses_the_wall_fit():
    from piml_amd import calibrate
    a = calibrate.get_args(['--data', 'clip.npy', '--match-stats', '--fit', 'A,B,Aw,Bw', '--init', 'Aw=50,Bw=-5',
                            '--wall-cutoff', '1.5'])
    assert a.fit == ('A', 'B', 'Aw', 'Bw') and a.init == {'Aw': 50.0, 'Bw': -5.0} and a.wall_cutoff == 1.5
    assert a.match == ('crowd', 'pairs', 'obstacles')
    a = calibrate.get_args(['--data', 'clip.npy', '--match-stats'])
    assert a.fit == calibrate.PARAM_NAMES and a.match == ('crowd', 'pairs') and a.wall_cutoff is None
    for argv in (['--match-stats', '--fit', 'Aw,Bw'], ['--match-stats', '--fit', 'Aw', '--init', 'Aw=50'],
                 ['--fit', 'Aw,Bw', '--init', 'Aw=50,Bw=-5'], ['--match-stats', '--wall-cutoff', '2'],
                 ['--match-stats', '--fit', 'Cw']):
        with pytest.raises(SystemExit):
            calibrate.get_args(['--data', 'clip.npy'] + argv)


def _obstacle_stats(hits, contacts, clear):
    """fabricated ObstacleStats of one member: 10 tracks, 100 focal agent-frames"""
    from piml_amd import obstaclestats as OS
    arrays = {k: np.zeros(1, np.int64) for k in OS.COUNTS + ('tracks', 'tracks_hit', 'tracks_contact')}
    arrays.update({k: np.zeros((1, 5), np.int64) for k in OS.R_ROWS + ('trk_min_hist',)})
    arrays['min_ttc'] = np.zeros((1, 4), np.int64)
    arrays['focal'][:], arrays['steps'][:], arrays['tracks'][:] = 100, 90, 10
    arrays['tracks_hit'][:], arrays['contact'][:] = hits, contacts
    arrays['clear'][0] = clear
    opts = dict(dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.5, r_bins=4, tau_bin=1.0, tau_bins=3, box=None, frames=None,
                n_obstacles=7, obstacles_hash='x')
    return OS.ObstacleStats(arrays, opts)


def test_stats_objective_with_the_obstacle_side():
    from piml_amd import calibrate
    assert calibrate.OBJECTIVE_KEYS['obstacles'] == ('hit_track_fraction_diff', 'contact_rate_diff', 'clearance_l1')
    sim, ref = _obstacle_stats(4, 30, [50, 30, 10, 10, 0]), _obstacle_stats(1, 10, [10, 30, 50, 10, 0])
    J, terms = calibrate.stats_objective(obstacles=sim, ref_obstacles=ref)
    assert terms['hit_track_fraction_diff'] == pytest.approx(0.3) and terms['contact_rate_diff'] == pytest.approx(0.2)
    assert terms['clearance_l1'] == pytest.approx(0.8)
    assert J == pytest.approx(0.3 + 0.2 + 0.8)
    J2, _ = calibrate.stats_objective(obstacles=sim, ref_obstacles=ref, weights={'clearance_l1': 0.0, 'contact_rate_diff': 2.0})
    assert J2 == pytest.approx(0.3 + 0.4)
    assert calibrate.stats_objective(obstacles=ref, ref_obstacles=ref)[0] == 0.0
    with pytest.raises(ValueError):
        calibrate.stats_objective(obstacles=sim)                 # no reference: no side
    with pytest.raises(ValueError):
        calibrate.stats_objective(obstacles=sim, ref_obstacles=ref, weights={'min_ttc_l1': 1.0})


def test_stats_fit_moves_the_wall_constants_within_their_bounds():
    from piml_amd import calibrate
    seen = []

    def evaluate(cands):
        seen.extend(cands)
        return [(c['Aw'] - 20.0) ** 2 / 400.0 + (c['Bw'] + 2.0) ** 2 for c in cands]
    res = calibrate.calibrate_mlapm_to_stats(None, None, init={'Aw': 50.0, 'Bw': -5.0}, fit=('Aw', 'Bw'), population=12,
                                             generations=12, evaluate=evaluate, wall_cutoff=1.5)
    assert all(c['Aw'] >= 0.0 and c['Bw'] <= 0.0 for c in seen) and all(c['A'] == 7.55 and c['tau'] == 0.5 for c in seen)
    assert res.params['wall_cutoff'] == 1.5 and res.final_loss < res.initial_loss
    assert abs(res.params['Aw'] - 20.0) < abs(50.0 - 20.0) and abs(res.params['Bw'] + 2.0) < 3.0
    assert all(a >= b for a, b in zip(res.history, res.history[1:]))
    # the default bounds hold where the optimum lies beyond them
    res = calibrate.calibrate_mlapm_to_stats(None, None, init={'Aw': 1.0, 'Bw': -0.5}, fit=('Aw', 'Bw'), population=8,
                                             generations=6, sigma=2.0,
                                             evaluate=lambda cs: [c['Aw'] - c['Bw'] for c in cs])
    assert res.params['Aw'] >= 0.0 and res.params['Bw'] <= 0.0
    # a fixed wall term is carried through; the plain fit has no wall keys
    res = calibrate.calibrate_mlapm_to_stats(None, None, init={'Aw': 50.0, 'Bw': -5.0}, fit=('A',), population=4, generations=2,
                                             evaluate=lambda cs: [abs(c['A'] - 5.0) for c in cs])
    assert res.params['Aw'] == 50.0 and res.params['Bw'] == -5.0 and res.params['wall_cutoff'] == 2.0
    res = calibrate.calibrate_mlapm_to_stats(None, None, fit=('A',), population=4, generations=2,
                                             evaluate=lambda cs: [abs(c['A'] - 5.0) for c in cs])
    assert not {'Aw', 'Bw', 'wall_cutoff'} & set(res.params)
    for kw in (dict(fit=('Aw',)), dict(fit=('Aw', 'Bw')), dict(fit=('Aw', 'Bw'), init={'Aw': 50.0}),
               dict(fit=('A',), init={'Bw': -5.0}), dict(fit=('Aw', 'Bw'), init={'Aw': -1.0, 'Bw': -5.0}),
               dict(fit=('Aw', 'Bw'), init={'Aw': 50.0, 'Bw': -5.0}, wall_cutoff=0.0)):
        with pytest.raises(ValueError):
            calibrate.calibrate_mlapm_to_stats(None, None, population=4, generations=1, evaluate=lambda cs: [0.0] * len(cs), **kw)
    assert math.isfinite(res.final_loss)
