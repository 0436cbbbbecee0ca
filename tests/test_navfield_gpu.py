"""GPU: the floor field.  piml_nav_relax against the numpy float32 restatement (nav_ref.py), bit for bit -- at its fixed point
on grids smaller than the halo, across tile edges and through several launches, and after ONE launch from a state that has
not converged (the temporal blocking's exactness) --, a captured batch against the eager one, and piml_nav_direction against
the restated three-branch lookup: branch and neighbour exact, the direction to 1e-5."""
import functools

import numpy as np
import pytest
import torch

import nav_ref as REF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(blocked (gy, gx), goal (G, gy, gx)) uint8"""
    if name == '1x1':                                            # gate 0's goal is the cell; gate 1 has none
        goal = np.zeros((2, 1, 1), np.uint8)
        goal[0, 0, 0] = 1
        return np.zeros((1, 1), np.uint8), goal
    if name == 'strip':                                          # 1 x 40: the halo is wider than the grid; a cut at x = 30
        blocked, goal = np.zeros((1, 40), np.uint8), np.zeros((1, 1, 40), np.uint8)
        blocked[0, 30] = 1
        goal[0, 0, 3] = 1
        return blocked, goal
    if name == 'u_shape':
        return REF.u_shape_case()
    blocked, goal = np.zeros((65, 65), np.uint8), np.zeros((1, 65, 65), np.uint8)      # 'empty': 3 x 3 tiles
    goal[0, 32, 32] = 1
    return blocked, goal


@functools.lru_cache(maxsize=None)
def fixed_point(name):
    """the restatement's, computed once"""
    blocked, goal = case(name)
    u, n = REF.solve(blocked, goal)
    u.setflags(write=False)
    return u, n


def on_gpu(name):
    blocked, goal = case(name)
    return torch.from_numpy(blocked).to(DEV), torch.from_numpy(goal).to(DEV)


@pytest.mark.parametrize('name', ['1x1', 'strip', 'u_shape', 'empty'])
def test_fixed_point_is_the_restatements(name):
    from piml_amd import ops_scenario
    want, n = fixed_point(name)
    blocked, goal = on_gpu(name)
    u, steps = ops_scenario.nav_relax(blocked, goal)
    batch = ops_scenario.NAV_BATCH * ops_scenario.NAV_STEPS
    assert steps == (-(-n // batch) + 1) * batch                # stopped at the first batch that changed nothing
    print(f'\n[nav] {name}: {want.shape[2]} x {want.shape[1]}, {want.shape[0]} gates, fixed point after {n} steps, {steps} queued')
    assert tuple(u.shape) == want.shape and u.dtype == torch.float32
    assert np.array_equal(bits(u.cpu().numpy()), bits(want))
    if name == '1x1':
        assert u.flatten().tolist() == [0.0, float('inf')]
    if name == 'strip':
        assert u[0, 0, :30].tolist() == [abs(x - 3.0) for x in range(30)] and torch.isinf(u[0, 0, 30:]).all()
    if name == 'u_shape':
        assert n > 4 * ops_scenario.NAV_STEPS                    # the path runs through several launches
        field = ops_scenario.NavField(u, blocked, goal, 0.0, 0.0, 0.25, 2.0)
        for g in range(2):
            r = field.reachable(g)
            assert r.dtype == torch.bool and not bool(r[20, 30]) and bool(r[20, 28]) and bool(r[20, 32])
            assert int(r.sum()) == int((case(name)[0] == 0).sum()) - 1 + (1 if g == 1 else 0)      # (gate 1's blocked goal)
        got = field.to_numpy()
        assert np.array_equal(bits(got.u), bits(want)) and (got.gx, got.gy, got.G) == (33, 34, 2)


@pytest.mark.parametrize('name,before', [('u_shape', 5), ('empty', 11), ('strip', 2)])
def test_one_launch_is_eight_steps_of_the_whole_plane(name, before):
    """from a state that has not converged: one launch == 8 restated steps, three launches == 24, bit for bit"""
    from piml_amd import ops_scenario
    blocked, goal = case(name)
    u0 = REF.steps(REF.start(goal), blocked, goal, before)
    assert not np.array_equal(bits(REF.jacobi_step(u0, blocked, goal)), bits(u0))
    gb, gg = on_gpu(name)
    start = torch.from_numpy(u0).to(DEV)
    for launches in (1, 3):
        u, steps = ops_scenario.nav_relax(gb, gg, u=start, launches=launches)
        assert steps == 8 * launches
        want = REF.steps(u0, blocked, goal, 8 * launches)
        assert np.array_equal(bits(u.cpu().numpy()), bits(want)), (name, launches)
        assert not np.array_equal(bits(want), bits(fixed_point(name)[0])) or name == 'strip'      # still on its way
    assert np.array_equal(bits(start.cpu().numpy()), bits(u0))   # the start is not written
    # a state that disagrees with the fixed cells is stepped from the fixed values
    wrong = torch.full_like(start, 7.0)
    u, _ = ops_scenario.nav_relax(gb, gg, u=wrong, launches=1)
    assert np.array_equal(bits(u.cpu().numpy()), bits(REF.steps(np.full_like(u0, 7.0), blocked, goal, 8)))


def test_captured_batch_equals_the_eager_batch():
    from piml_amd import _lib, hip_graphs_safe, ops_scenario
    from piml_amd.ops import _ptr, _stream
    assert hip_graphs_safe()
    blocked, goal = case('u_shape')
    gb, gg = on_gpu('u_shape')
    u0 = torch.from_numpy(REF.start(goal)).to(DEV)
    L = _lib.lib()

    def batch(a, b, changed):
        _lib.check(L.piml_nav_relax(_ptr(gb), _ptr(gg), _ptr(a), _ptr(b), 2, 33, 34, ops_scenario.NAV_BATCH, _ptr(changed),
                                    _stream()), 'piml_nav_relax')
    a1, b1, c1 = u0.clone(), torch.empty_like(u0), torch.zeros(2, device=DEV, dtype=torch.int32)
    batch(a1, b1, c1)
    a2, b2, c2 = u0.clone(), torch.empty_like(u0), torch.zeros(2, device=DEV, dtype=torch.int32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch(a2, b2, c2)
    a2.copy_(u0)
    c2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and c1.tolist() == c2.tolist() == [1, 1]
    assert np.array_equal(bits(a2.cpu().numpy()), bits(fixed_point('u_shape')[0]))    # 128 steps are enough here
    c2.zero_()
    graph.replay()                                               # at the fixed point nothing changes
    torch.cuda.synchronize()
    assert c2.tolist() == [0, 0] and torch.equal(a1.view(torch.int32), a2.view(torch.int32))


# ---- the lookup ----

X0, Y0, CELL, NEAR = -1.0, 2.0, 0.25, 2.0


@functools.lru_cache(maxsize=None)
def lookup_rows():
    """(P (n, 2), gate (n), dest (n, 2)) float32 / int32 over the U-shaped field with origin (X0, Y0)"""
    rng = np.random.default_rng(7)
    gx, gy = 33, 34
    x0, y0, c = f32(X0), f32(Y0), f32(CELL)
    ii, jj = np.meshgrid(np.arange(gx), np.arange(gy))
    rows = []
    for fx, fy in ((0.5, 0.5), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):       # centres and the four quadrants:
        rows.append(np.stack([x0 + (ii.ravel() + f32(fx)) * c, y0 + (jj.ravel() + f32(fy)) * c], 1))   # blocked cells, beside them,
    kx, ky = rng.integers(0, gx + 1, 300), rng.integers(0, gy + 1, 300)                       # near the gates, the enclosed cell
    edge_x, edge_y = x0 + kx.astype(f32) * c, y0 + ky.astype(f32) * c                         # cell edges, the border included
    other = rng.uniform([X0, Y0], [X0 + gx * CELL, Y0 + gy * CELL], (300, 2)).astype(f32)
    rows += [np.stack([edge_x, other[:, 1]], 1), np.stack([other[:, 0], edge_y], 1), np.stack([edge_x, edge_y], 1)]
    rows.append(rng.uniform([X0 - 0.6, Y0 - 0.6], [X0 + gx * CELL + 0.6, Y0 + gy * CELL + 0.6], (1500, 2)).astype(f32))   # in and out
    rows.append(np.array([[np.nan, 3.0], [3.0, np.nan], [np.nan, np.nan], [np.inf, 3.0], [3.0, -np.inf]], f32))
    P = np.concatenate(rows).astype(f32)
    gate = rng.integers(0, 2, P.shape[0]).astype(np.int32)
    gate[::211] = rng.choice([-1, 2, 64, -2 ** 31, 2 ** 31 - 1], gate[::211].shape[0])        # gates that do not exist
    dest = rng.uniform([X0, Y0], [X0 + gx * CELL, Y0 + gy * CELL], P.shape).astype(f32)
    dest[5::97] = P[5::97]                                       # dest == p: the 1e-12 clamp
    return P, gate, dest


@functools.lru_cache(maxsize=None)
def lookup_want():
    P, gate, dest = lookup_rows()
    return REF.direction(fixed_point('u_shape')[0], X0, Y0, CELL, NEAR, P, gate, dest)


def lookup_field():
    from piml_amd import ops_scenario
    gb, gg = on_gpu('u_shape')
    u = torch.from_numpy(np.array(fixed_point('u_shape')[0])).to(DEV)
    return ops_scenario.NavField(u, gb, gg, X0, Y0, CELL, NEAR)


def test_lookup_matches_the_restatement():
    from piml_amd import ops_scenario
    P, gate, dest = lookup_rows()
    e_want, b_want, k_want = lookup_want()
    field = lookup_field()
    tp, tg, td = (torch.from_numpy(x).to(DEV) for x in (P, gate, dest))
    e, b, k = ops_scenario.nav_direction(tp, tg, td, field, return_branch=True)
    assert e.shape == tp.shape and b.dtype == k.dtype == torch.int32
    b, k, e = b.cpu().numpy(), k.cpu().numpy(), e.cpu().numpy().astype(np.float64)
    counts = np.bincount(b_want, minlength=3)
    print(f'\n[nav] lookup: {len(P)} rows, branches {counts.tolist()}, neighbours {np.bincount(k_want[k_want >= 0], minlength=8).tolist()}')
    assert np.array_equal(b, b_want), np.flatnonzero(b != b_want)[:10]
    assert np.array_equal(k, k_want), np.flatnonzero(k != k_want)[:10]
    fin = np.isfinite(e_want).all(1)
    assert np.array_equal(np.isfinite(e).all(1), fin)
    err = np.abs(e[fin] - e_want[fin]).max()
    print(f'[nav] lookup: largest direction error {err:.3g}')
    assert err <= 1e-5
    assert np.abs(np.hypot(e[fin & (b_want > 0), 0], e[fin & (b_want > 0), 1]) - 1.0).max() <= 1e-5
    # every case of the list is there
    assert counts.min() > 100 and set(k_want[b_want == 2].tolist()) >= {0, 1, 2, 3}
    u = fixed_point('u_shape')[0]
    q = np.floor((P - f32([X0, Y0])) / f32(CELL))
    inside = np.isfinite(q).all(1) & (q[:, 0] >= 0) & (q[:, 0] < 33) & (q[:, 1] >= 0) & (q[:, 1] < 34)
    ok_gate = (gate >= 0) & (gate < 2)
    assert (b_want[~inside] == 0).all() and (~inside).sum() > 300 and (b_want[~ok_gate] == 0).all() and (~ok_gate).sum() > 10
    cx, cy = q[inside & ok_gate, 0].astype(int), q[inside & ok_gate, 1].astype(int)
    uc = u[gate[inside & ok_gate], cy, cx]
    bb = b_want[inside & ok_gate]
    assert (bb[np.isinf(uc)] == 0).all() and np.isinf(uc).sum() > 300       # blocked and unreachable cells
    assert (bb[uc <= NEAR] == 0).all() and (uc <= NEAR).sum() > 20 and (bb[np.isfinite(uc) & (uc > NEAR)] > 0).all()
    enclosed = (cx == 30) & (cy == 20)
    assert enclosed.sum() >= 5 and (bb[enclosed] == 0).all()
    # branch 2 with a diagonal that would have won had it not been skipped
    _, b_cut, k_cut = REF.direction(u, X0, Y0, CELL, NEAR, P[b_want == 2], gate[b_want == 2], dest[b_want == 2], skip_rule=False)
    assert (b_cut == 2).all() and (k_cut != k_want[b_want == 2]).sum() >= 4
    # branch 0 is the frame's own line
    straight = (b_want == 0) & np.isfinite(P).all(1)
    d = (dest - P)[straight].astype(f32)
    fma = (d[:, 1].astype(np.float64) * d[:, 1] + (d[:, 0] * d[:, 0]).astype(f32)).astype(f32)     # norm2: sqrt(fma(y, y, x x))
    n = np.maximum(np.sqrt(fma), f32(1e-12))
    assert np.array_equal(bits(e[straight].astype(f32)), bits((d / n[:, None]).astype(f32)))


def test_lookup_shapes():
    from piml_amd import ops_scenario
    P, gate, dest = lookup_rows()
    field = lookup_field()
    tp, tg, td = (torch.from_numpy(x[:15]).to(DEV) for x in (P[1000:], gate[1000:], dest[1000:]))
    flat = ops_scenario.nav_direction(tp, tg, td, field, return_branch=True)
    lead = ops_scenario.nav_direction(tp.view(3, 5, 2), tg.view(3, 5), td.view(3, 5, 2), field, return_branch=True)
    assert lead[0].shape == (3, 5, 2) and lead[1].shape == lead[2].shape == (3, 5)
    assert all(torch.equal(a.view(torch.int32).flatten(), b.view(torch.int32).flatten()) for a, b in zip(flat, lead))
    only = ops_scenario.nav_direction(tp, tg.long(), td, field)                 # any integer gate; without the branch
    assert torch.equal(only.view(torch.int32), flat[0].view(torch.int32))
    empty = ops_scenario.nav_direction(tp[:0], tg[:0], td[:0], field, return_branch=True)
    assert empty[0].shape == (0, 2) and empty[1].shape == empty[2].shape == (0,)
    for bad in ((tp, tg[:3], td), (tp, tg.float(), td), (tp[:, :1], tg, td[:, :1]), (tp, tg, td[:3]), (tp.cpu(), tg, td)):
        with pytest.raises((ValueError, RuntimeError)):
            ops_scenario.nav_direction(*bad, field)
    with pytest.raises(TypeError):
        ops_scenario.nav_direction(tp, tg, td, object())


def test_field_of_a_floor_plan():
    """nav_field end to end on two rooms and a door: blocked cells by the wall operator's exact distance, goal cells free,
    the field the restatement's, and the way from the left room to the right gate leads through the door"""
    from piml_amd import ops_scenario, scenarios
    walls = [[[5.0, -2.0], [5.0, 4.5]], [[5.0, 5.5], [5.0, 12.0]]]
    gates = [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]
    sc = scenarios.floorplan_scenario(walls, gates, gate_points=50).to(DEV)
    field = ops_scenario.nav_field(sc, cell=0.25, clearance=0.3, device=DEV)
    h = ops_scenario.nav_grid_host(sc, 0.25)
    got = field.to_numpy()
    assert (got.gx, got.gy, got.x0, got.y0, got.cell, got.near) == (h.gx, h.gy, h.x0, h.y0, 0.25, 2.0)
    obs = sc.obstacles.cpu().numpy().astype(np.float64)
    d2 = ((h.centres.reshape(-1, 1, 2).astype(np.float64) - obs[None]) ** 2).sum(-1).min(1).reshape(h.gy, h.gx)
    sure = np.abs(np.sqrt(d2) - 0.3) > 1e-4                      # (cells within float32 rounding of the clearance: either way)
    assert np.array_equal((got.blocked != 0)[sure], (d2 < 0.09)[sure]) and np.array_equal(got.goal, h.goal)
    assert not (got.blocked[None] & got.goal).any() and got.blocked.sum() > 100
    want, n = REF.solve(got.blocked, got.goal)
    assert np.array_equal(bits(got.u), bits(want)) and field.iterations >= n
    print(f'\n[nav] two rooms: {got.gx} x {got.gy} cells, fixed point after {n} steps, {field.iterations} queued')
    # from the middle of the left room to the right gate: farther than the straight line, and downhill through the door
    cell_of = lambda x, y: (int(np.floor((f32(y) - f32(h.y0)) / f32(0.25))), int(np.floor((f32(x) - f32(h.x0)) / f32(0.25))))
    start = cell_of(2.0, 1.0)
    assert want[1][start] * 0.25 > np.hypot(3.0, 4.0) + np.hypot(5.0, 3.5) - 1.0
    door = cell_of(5.0, 5.0)
    assert np.isfinite(want[:, door[0], door[1]]).all() and np.isinf(want[:, cell_of(5.0, 2.0)[0], cell_of(5.0, 2.0)[1]]).all()
    assert want[1][start] > want[1][door] > want[1][cell_of(8.0, 2.0)]
