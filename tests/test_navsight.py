"""No GPU: the any-angle floor field on its numpy restatement (navsight_ref.py) and on the host side.  The propagation on an
empty grid and round a U-shaped wall (fixed points, parent chains, w against the first-order field), the soundness of the
table by brute force in float64 (no segment from a point of a cell to its parent's centre enters a blocked cell), the sight
test's symmetries and its two defining cases (a diagonal pinch is never visible, a run along a wall face is), the lookup's
branch 3 in open space, and the new names' host checks: NavField, simulate's arguments, the C entries' refusals."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref
import navsight_ref as REF
from conftest import REPO

f32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def solved(name):
    """(blocked, goal, w, parent, steps) of the restatement, computed once and read-only"""
    if name == 'empty':
        blocked, goal = np.zeros((33, 33), np.uint8), np.zeros((1, 33, 33), np.uint8)
        goal[0, 16, 16] = 1
    elif name == 'u_wall':
        blocked, goal = REF.u_wall_case()
    else:
        blocked, goal = nav_ref.u_shape_case()
    w, parent, n = REF.solve(blocked, goal)
    for a in (blocked, goal, w, parent):
        a.setflags(write=False)
    return blocked, goal, w, parent, n


# ---- 1. the propagation ----

def test_empty_grid_every_parent_is_the_goal_and_w_is_the_distance():
    blocked, goal, w, parent, n = solved('empty')
    assert n == 16
    assert (parent == 16 * 33 + 16).all()
    yy, xx = np.mgrid[:33, :33]
    want = np.sqrt(((xx - 16) ** 2 + (yy - 16) ** 2).astype(f32)).astype(f32)
    assert np.array_equal(bits(w[0]), bits(want))
    # one more step changes nothing, and the step before the last did
    assert REF.same(REF.jacobi_step(w, parent, blocked, goal), (w, parent))
    assert not REF.same(REF.steps(blocked, goal, 15), (w, parent))


def test_u_wall_chains_and_lengths():
    blocked, goal, w, parent, n = solved('u_wall')
    assert n == 32
    assert REF.chain(parent[0], (28, 16)) == [(21, 25), (9, 25), (9, 23), (16, 16)]
    assert abs(float(w[0, 16, 28]) - 35.301247) < 1e-5
    free = blocked == 0
    u, _ = nav_ref.solve(blocked, goal)
    assert abs(float(u[0, 16, 28]) - 36.76) < 0.01
    assert (w[0][free] <= u[0][free] + 1e-4).all() and np.isfinite(w[0][free]).all()
    assert np.isinf(w[0][~free]).all() and (parent[0][~free] == -1).all()
    longest = 0
    for y, x in zip(*np.nonzero(free)):
        ch = REF.chain(parent[0], (int(x), int(y)))
        longest = max(longest, len(ch))
        ws = [float(w[0, y, x])] + [float(w[0, cy, cx]) for cx, cy in ch]
        if (x, y) == (16, 16):
            assert ch == [] and ws == [0.0]
            continue
        assert ch and ch[-1] == (16, 16), (x, y, ch)
        assert all(a > b for a, b in zip(ws, ws[1:])), (x, y, ws)             # w strictly falls along the chain
    assert longest == 4


def test_enclosed_cell_and_blocked_goal():
    """nav_ref's 33 x 34 case: the free cell (30, 20) walled in on all four sides keeps (+inf, -1) for both gates; gate 1's
    goal on the blocked cell (8, 5) is free for gate 1 (a source of its field) and a wall for gate 0"""
    blocked, goal, w, parent, n = solved('u_shape')
    assert blocked[20, 30] == 0
    assert np.isinf(w[:, 20, 30]).all() and (parent[:, 20, 30] == -1).all()
    assert np.isfinite(w[:, 20, 28]).all() and np.isfinite(w[:, 20, 32]).all()
    assert w[1, 5, 8] == 0 and parent[1, 5, 8] == 5 * 33 + 8 and np.isinf(w[0, 5, 8]) and parent[0, 5, 8] == -1
    assert (parent[1] == 5 * 33 + 8).sum() > 1                   # cells whose string ends on it
    u, _ = nav_ref.solve(blocked, goal)
    assert np.array_equal(np.isfinite(w), np.isfinite(u))        # the same cells are reachable
    # (w <= u does not hold here as it does round the U wall above: a string through cell centres rounds a corner half a cell
    # out, and the first-order front does not)


# ---- 2. soundness ----

def test_no_segment_to_a_parents_centre_enters_a_blocked_cell():
    """13 points of every free cell with a parent (corners, edge midpoints, centre, 4 seeded random points), the segment to the
    parent's centre sampled every 1/8 cell in float64: no sample lies strictly inside (by more than 1e-9) a blocked cell or
    outside the grid.  1051 cells x 13 = 13 663 segments"""
    blocked, goal, w, parent, n = solved('u_wall')
    rng = np.random.default_rng(11)
    fixed = [(a, b) for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0)]
    pad = np.pad(blocked != 0, 1, constant_values=True)
    segments = bad = 0
    for y, x in zip(*np.nonzero(blocked == 0)):
        q = int(parent[0, y, x])
        if q < 0 or q == y * 33 + x:
            continue
        T = np.array([q % 33 + 0.5, q // 33 + 0.5])
        for fx, fy in fixed + [tuple(r) for r in rng.random((4, 2))]:
            p = np.array([x + fx, y + fy])
            k = int(np.ceil(np.hypot(*(T - p)) * 8)) + 1
            s = p[None] + np.linspace(0.0, 1.0, k)[:, None] * (T - p)[None]
            cell = np.floor(s)
            frac = s - cell
            inner = ((frac > 1e-9) & (frac < 1 - 1e-9)).all(1)
            ix, iy = np.clip(cell[:, 0].astype(int), -1, 33), np.clip(cell[:, 1].astype(int), -1, 33)
            bad += int((inner & pad[iy + 1, ix + 1]).any())
            segments += 1
    print(f'\n[navsight] soundness: {bad} of {segments} segments enter a blocked cell')
    assert segments == 13663 and bad == 0


# ---- 3. the sight test ----

def test_visible_is_symmetric_under_the_grids_symmetries():
    rng = np.random.default_rng(5)
    n = 12
    mask = rng.random((n, n)) < 0.2
    free = [(int(x), int(y)) for y, x in zip(*np.nonzero(~mask))]
    pairs = [(free[i], free[j]) for i, j in rng.integers(0, len(free), (150, 2))]
    base = [REF.visible(mask, c, q) for c, q in pairs]
    assert 30 < sum(base) < 130                                  # both answers occur
    for flip_x in (False, True):
        for flip_y in (False, True):
            for swap in (False, True):
                def T(c):
                    x, y = (n - 1 - c[0] if flip_x else c[0]), (n - 1 - c[1] if flip_y else c[1])
                    return (y, x) if swap else (x, y)
                m = mask[::-1] if flip_y else mask
                m = m[:, ::-1] if flip_x else m
                m = m.T if swap else m
                assert all(m[T(c)[1], T(c)[0]] == mask[c[1], c[0]] for c in free[:20])
                assert [REF.visible(m, T(c), T(q)) for c, q in pairs] == base, (flip_x, flip_y, swap)


def test_a_pinch_is_not_visible_and_a_wall_face_is():
    mask = np.zeros((12, 12), bool)
    mask[5, 5] = mask[6, 6] = True                               # blocked (5, 5) and (6, 6)
    assert not REF.visible(mask, (5, 6), (6, 5)) and not REF.visible(mask, (6, 5), (5, 6))
    assert not REF.visible(mask, (4, 7), (7, 4))                 # the same pinch from further away
    assert REF.visible(mask, (5, 6), (5, 9)) and REF.visible(mask, (4, 4), (4, 9))
    wall = np.zeros((12, 12), bool)
    wall[4, 2:10] = True                                         # a wall along y = 4
    assert REF.visible(wall, (2, 5), (9, 5)) and REF.visible(wall, (9, 3), (1, 3))       # along either face
    assert REF.visible(wall, (1, 5), (10, 5)) and not REF.visible(wall, (1, 5), (10, 3))
    assert not REF.visible(wall, (3, 5), (4, 3)) and not REF.visible(wall, (0, 5), (2, 3))
    assert REF.visible(wall, (0, 5), (1, 3))                     # round the end of the wall, through free cells only
    border = np.zeros((6, 6), bool)
    assert REF.visible(border, (0, 0), (5, 0)) and REF.visible(border, (0, 0), (0, 5)) and REF.visible(border, (0, 0), (5, 5))
    # the integer test against the definition in rationals.  The t that satisfy it form an interval whose ends are among 0, 1
    # and the four bounds, so if there is one, 0, 1 or the midpoint of two of those values is one
    from fractions import Fraction as F
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(600):
        ax, ay, Dx, Dy = (int(v) for v in rng.integers(-6, 7, 4))
        ends = [F(0), F(1)] + [F(2 * a + s, 2 * D + r) for a, D in ((ax, Dx), (ay, Dy)) for s, r in ((-2, -1), (2, 1))]
        ts = ends + [(p + q) / 2 for i, p in enumerate(ends) for q in ends[i + 1:]]
        brute = any(0 <= t <= 1 and abs(ax - t * Dx) < 1 - t / 2 and abs(ay - t * Dy) < 1 - t / 2 for t in ts)
        assert REF.obstructs(ax, ay, Dx, Dy) == brute, (ax, ay, Dx, Dy)
        seen.add(brute)
    assert seen == {False, True}


# ---- 4. the lookup in open space ----

def test_branch_3_points_at_the_goal_where_the_gradient_is_off():
    """empty 33 x 33 grid, cell 0.25, every cell beyond near = 2, nine points per cell: branch 3 is the straight line to the
    goal cell's centre to 1e-6; the bilinear branch's mean and largest angle off that line on the same points are printed
    (4.66 and 25.1 degrees here; DESIGN 4.31 quotes 3 and 16 from its own prototype)"""
    blocked, goal, w, parent, n = solved('empty')
    u, _ = nav_ref.solve(blocked, goal)
    x0, y0, cell, near = f32(-1.0), f32(2.0), f32(0.25), 2.0
    ii, jj = np.meshgrid(np.arange(33), np.arange(33))
    P = np.concatenate([np.stack([x0 + (ii.ravel() + f32(fx)) * cell, y0 + (jj.ravel() + f32(fy)) * cell], 1)
                        for fx in (0.25, 0.5, 0.75) for fy in (0.25, 0.5, 0.75)]).astype(f32)
    beyond = np.tile((u[0] > near).ravel(), 9)
    P = P[beyond]
    gate, dest = np.zeros(len(P), np.int32), np.zeros_like(P)
    base = nav_ref.direction(u, x0, y0, cell, near, P, gate, dest)
    e, b, k = REF.direction(u, parent, x0, y0, cell, near, P, gate, dest, base=base)
    assert (b == 3).all() and (k == -1).all() and len(P) == 9 * int((u[0] > near).sum()) > 9000
    centre = np.array([float(x0) + 16.5 * 0.25, float(y0) + 16.5 * 0.25])
    line = centre[None] - P.astype(np.float64)
    line /= np.hypot(line[:, 0], line[:, 1])[:, None]
    assert np.abs(e - line).max() <= 1e-6
    bil = base[1] == 1                                           # without the table: bilinear but in the outer half of the
    assert bil.sum() > 0.9 * len(P) and (base[1][~bil] == 2).all()         # border cells, which have no four centres around
    ang = np.degrees(np.arccos(np.clip((base[0] * line).sum(1), -1, 1)))[bil]
    far = (np.hypot(*((P.astype(np.float64) - centre[None]) / 0.25).T) > 8)[bil]
    print(f'\n[navsight] open space, {len(P)} points: the bilinear branch ({int(bil.sum())} of them) is off the line by '
          f'{ang.mean():.2f} deg on average, {ang.max():.2f} deg at worst ({ang[far].max():.2f} beyond 8 cells); the sight branch by '
          f'{np.degrees(np.arccos(np.clip((e * line).sum(1), -1, 1))).max():.2g} deg')
    # degrees against rounding: the figures are printed, not pinned
    assert ang.mean() > 1.0 and ang.max() > 5.0


# ---- 5. the host side ----

def test_navfield_members():
    import torch
    from piml_amd import _lib, ops_scenario
    u = torch.zeros(2, 4, 5)
    z = torch.zeros(2, 4, 5, dtype=torch.uint8)
    old = ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 0.25, 2.0)                 # the seven positional arguments
    assert old.parent is None and old.w is None and old.sight_desc is None and old.sight_iterations == 0
    assert not hasattr(old.to_numpy(), 'parent') and old.to_numpy().u.shape == (2, 4, 5)
    assert ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 0.25, 2.0, 0.3, 24).iterations == 24
    parent = torch.full((2, 4, 5), -1, dtype=torch.int32)
    new = ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 0.25, 2.0, 0.3, 24, w=u.clone(), parent=parent, sight_iterations=64)
    assert isinstance(new.sight_desc, _lib.NavSight) and new.sight_desc.parent == parent.data_ptr()
    assert (new.sight_desc.G, new.sight_desc.gx, new.sight_desc.gy) == (2, 5, 4) and new.sight_iterations == 64
    got = new.to_numpy()
    assert got.parent.dtype == np.int32 and (got.parent == -1).all() and got.w.shape == (2, 4, 5)
    with pytest.raises(TypeError):
        ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 0.25, 2.0, 0.3, 24, u, parent)       # keyword-only
    for bad in (parent.long(), parent[:1], parent.float()):
        with pytest.raises(ValueError, match='parent'):
            ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 0.25, 2.0, parent=bad)
    assert ops_scenario.nav_wants_sight(True) is False and ops_scenario.nav_wants_sight('sight') is True
    assert ops_scenario.nav_wants_sight(old) is False and ops_scenario.nav_wants_sight(new) is True
    for bad in ('yes', 1, object()):
        with pytest.raises(TypeError):
            ops_scenario.nav_wants_sight(bad)
    # no CPU path
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_sight_relax(torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(1, 3, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops_scenario.nav_sight_relax(torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='sight=True'):
        ops_scenario.nav_direction(torch.zeros(1, 2), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2), old, sight=True)


def test_scenes_are_refused_before_any_state_with_the_sight_field_too():
    from piml_amd import scenarios
    from piml_amd.models import mlapm
    base = {'version': 'GC', 'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
    gc = scenarios.gc_scenario()
    sim = mlapm.MLAPM(**base)
    with pytest.raises(ValueError, match='route_max_iters'):
        sim.simulate_scenario(gc, 5, device='cpu', nav='sight')
    with pytest.raises(ValueError, match='gates'):
        sim.simulate_ensemble(scenarios.crosswalk_scenario(), 5, [0, 1], device='cpu', nav='sight')
    with pytest.raises(ValueError, match='route_max_iters'):
        mlapm.SweepRun(gc, 5, 1, [0], device='cpu', nav='sight')
    with pytest.raises(TypeError, match='sight'):
        sim.simulate_scenario(gc, 5, device='cpu', nav='lines')
    with pytest.raises(TypeError, match='sight'):
        mlapm.SweepRun(gc, 5, 1, [0], device='cpu', nav=2)


def test_command_line_arguments(tmp_path):
    from piml_amd import simulate
    own, _ = simulate.get_args(['--law', 'mlapm', '--scenario', 'gc', '--nav', '--nav-sight'])
    assert own.nav and own.nav_sight and own.nav_cell == 0.25
    own, _ = simulate.get_args(['--law', 'mlapm', '--scenario', 'gc', '--nav'])
    assert own.nav and not own.nav_sight
    plan = tmp_path / 'plan.json'
    plan.write_text(json.dumps({'walls': [[[5.0, -1.0], [5.0, 4.5]]], 'gates': [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]}))
    own, _ = simulate.get_args(['--law', 'mlapm', '--scene-plan', str(plan), '--nav', '--nav-sight', '--seeds', '0:2',
                                '--obstacle-stats', str(tmp_path / 'o.json')])
    assert own.nav_sight and own.plan is not None
    for argv in (['--law', 'mlapm', '--scenario', 'gc', '--nav-sight'], ['--law', 'mlapm', '--nav-sight'], ['--nav-sight'],
                 ['--law', 'pinnsf', '--nav', '--nav-sight'], ['--law', 'pinnsf', '--scene-plan', str(plan), '--nav-sight'],
                 ['--law', 'mlapm', '--scenario', 'crosswalk', '--nav', '--nav-sight']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)


# ---- 6. the C entries ----

def test_abi_lists_the_new_entries():
    from piml_amd import _lib
    header = open(os.path.join(REPO, 'include', 'piml_hip.h')).read()
    for name, n in (('piml_nav_sight_relax', 13), ('piml_nav_direction_sight', 10), ('piml_scenario_step_mlapm_sight', 14)):
        assert len(_lib.SIGNATURES[name]) == n and re.search(r'\bint %s\(' % name, header), name
    assert 'typedef struct piml_nav_sight {' in header
    assert ctypes.sizeof(_lib.NavSight) == 24 and _lib.NavSight.G.offset == 8
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols and a struct were only added


def test_argument_validation_without_gpu():
    """every refusal below comes before any HIP call: host buffers stand in for device ones and are never read"""
    from piml_amd import _lib
    L = _lib.lib()
    buf = [ctypes.create_string_buffer(64) for _ in range(8)]
    ptr = [ctypes.addressof(b) for b in buf]
    relax = lambda **kw: L.piml_nav_sight_relax(*[{**dict(blocked=ptr[0], goal=ptr[1], w_a=ptr[2], parent_a=ptr[3], w_b=ptr[4],
                                                         parent_b=ptr[5], cache=ptr[6], G=1, gx=2, gy=2, launches=0,
                                                         changed=ptr[7], stream=None), **kw}[k]
                                                  for k in ('blocked', 'goal', 'w_a', 'parent_a', 'w_b', 'parent_b', 'cache', 'G',
                                                            'gx', 'gy', 'launches', 'changed', 'stream')])
    assert relax() == 0                                          # launches == 0: a no-op, the set every refusal differs from
    for k in ('blocked', 'goal', 'w_a', 'parent_a', 'w_b', 'parent_b', 'cache', 'changed'):
        assert relax(**{k: None}) == 1, k
    assert relax(w_b=ptr[2]) == 1 and relax(parent_b=ptr[3]) == 1
    for kw in (dict(G=0), dict(G=65), dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025), dict(launches=-1)):
        assert relax(**kw) == 1, kw
    grid = _lib.NavGrid()
    grid.u, grid.G, grid.gx, grid.gy, grid.x0, grid.y0, grid.cell, grid.near = ptr[0], 2, 5, 4, 0.0, 0.0, 0.25, 2.0
    sight = _lib.NavSight()
    sight.parent, sight.G, sight.gx, sight.gy = ptr[1], 2, 5, 4
    look = lambda g, s, rows=0, out=ptr[2]: L.piml_nav_direction_sight(None, None, None, rows, g, s, out, None, None, None)
    assert look(ctypes.byref(grid), ctypes.byref(sight)) == 0    # rows == 0: success without a launch
    assert look(ctypes.byref(grid), None) == 1 and look(None, ctypes.byref(sight)) == 1
    assert look(ctypes.byref(grid), ctypes.byref(sight), out=None) == 1 and look(ctypes.byref(grid), ctypes.byref(sight), rows=-1) == 1
    assert look(ctypes.byref(grid), ctypes.byref(sight), rows=3) == 1            # NULL position with rows > 0
    for field, value in (('parent', None), ('G', 3), ('gx', 4), ('gy', 5)):
        bad = _lib.NavSight.from_buffer_copy(sight)
        setattr(bad, field, value)
        assert look(ctypes.byref(grid), ctypes.byref(bad)) == 1, field
    off = _lib.NavGrid.from_buffer_copy(grid)
    off.cell = 0.0
    assert look(ctypes.byref(off), ctypes.byref(sight)) == 1
    frame = lambda s, g, sd: L.piml_scenario_step_mlapm_sight(s, None, 1, ptr[3], None, None, None, None, None, g, sd, None, 0, None)
    assert frame(None, ctypes.byref(grid), ctypes.byref(sight)) == 1             # what _nav refuses: a NULL scene
    assert L.piml_scenario_step_mlapm_nav(None, None, 1, ptr[3], None, None, None, None, None, ctypes.byref(grid), None, 0, None) == 1
    assert frame(None, ctypes.byref(grid), None) == 1 and frame(None, None, ctypes.byref(sight)) == 1


# ---- 7. build ----

def test_sight_kernels_build_for_gfx950_without_scratch(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'navsight.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'navsight.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    report = re.findall(r'Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    names = [n for n, _ in report if n]
    scratch = [int(s) for _, s in report if s]
    assert len(names) == len(scratch), names
    assert any('nav_sight_relax_kernel' in n for n in names) and any('nav_direction_sight_kernel' in n for n in names), names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(int(x) == 0 for x in re.findall(r'LDS Size \[bytes/block\]: (\d+)', p.stderr))


def test_sight_kernels_do_not_spill():
    pytest.importorskip('msgpack')
    from piml_amd import _lib
    usage = _lib.kernel_resource_usage()
    for name in ('nav_sight_relax_kernel', 'nav_direction_sight_kernel', 'scenario_mlapm_sight_kernel<false, false>',
                 'scenario_mlapm_sight_kernel<false, true>', 'scenario_mlapm_sight_kernel<true, false>',
                 'scenario_mlapm_sight_kernel<true, true>'):
        assert name in usage, name
        assert usage[name]['vgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, (name, usage[name])
    nav, sight = usage['scenario_mlapm_nav_kernel<false, true>'], usage['scenario_mlapm_sight_kernel<false, true>']
    assert sight['vgprs'] <= nav['vgprs'] + 8 and sight['lds_bytes'] == nav['lds_bytes']
