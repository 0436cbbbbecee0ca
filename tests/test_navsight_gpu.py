"""GPU: the any-angle floor field.  piml_nav_sight_relax against the restatement (navsight_ref.py), bit for bit -- after one and
three steps from the start, at the driver's fixed point, through a captured batch --; piml_nav_direction_sight against the
restated lookup with branch 3; and the frame routed by the table (piml_scenario_step_mlapm_sight) in the pattern of
test_scenario_nav_gpu.py: the first frame against the plain frame steered to p + e, a table of -1 against the nav frame,
members / tables / captured replays against each other, two rooms and a door, an open room, the command line."""
import ctypes
import dataclasses
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nav_ref
import navsight_ref as REF
from conftest import REPO
from test_scenario_mlapm_gpu import LAW, _same, bits as tbits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


# ---- 1. the propagation ----

@functools.lru_cache(maxsize=None)
def case(name):
    """(blocked (gy, gx), goal (G, gy, gx)) uint8"""
    if name == '1x1':                                            # gate 0's goal is the cell; gate 1 has none
        goal = np.zeros((2, 1, 1), np.uint8)
        goal[0, 0, 0] = 1
        return np.zeros((1, 1), np.uint8), goal
    if name == 'strip':                                          # 1 x 40, the goal at one end, a cut at x = 30
        blocked, goal = np.zeros((1, 40), np.uint8), np.zeros((1, 1, 40), np.uint8)
        blocked[0, 30] = 1
        goal[0, 0, 0] = 1
        return blocked, goal
    if name == 'u_shape':                                        # 33 x 34, two gates, an enclosed cell, a goal on a blocked cell
        return nav_ref.u_shape_case()
    if name == 'random':                                         # 40 x 40, density 0.2: pinches, pockets, long chains
        rng = np.random.default_rng(3)
        blocked, goal = (rng.random((40, 40)) < 0.2).astype(np.uint8), np.zeros((1, 40, 40), np.uint8)
        goal[0, 20, 20] = 1
        blocked[20, 20] = 0
        return blocked, goal
    if name == 'u_wall':
        return REF.u_wall_case()
    blocked, goal = np.zeros((65, 65), np.uint8), np.zeros((1, 65, 65), np.uint8)      # 'empty': sight lines of up to 45 cells
    goal[0, 32, 32] = 1
    return blocked, goal


@functools.lru_cache(maxsize=None)
def sight_of(name):
    return REF.sights(*case(name))


@functools.lru_cache(maxsize=None)
def fixed_point(name):
    """the restatement's (w, parent, steps), computed once and read-only"""
    w, parent, n = REF.solve(*case(name), sight_of(name))
    w.setflags(write=False)
    parent.setflags(write=False)
    return w, parent, n


def on_gpu(name):
    blocked, goal = case(name)
    return torch.from_numpy(blocked).to(DEV), torch.from_numpy(goal).to(DEV)


@pytest.mark.parametrize('name', ['1x1', 'strip', 'u_shape', 'empty', 'random'])
def test_fixed_point_is_the_restatements(name):
    from piml_amd import ops_scenario
    w_want, p_want, n = fixed_point(name)
    gb, gg = on_gpu(name)
    w, parent, steps = ops_scenario.nav_sight_relax(gb, gg)
    batch = ops_scenario.NAV_SIGHT_BATCH
    print(f'\n[navsight] {name}: {w_want.shape[2]} x {w_want.shape[1]}, {w_want.shape[0]} gates, fixed point after {n} steps, '
          f'{steps} queued')
    assert steps == (-(-n // batch) + 1) * batch                # stopped at the first batch that changed nothing
    assert tuple(w.shape) == w_want.shape and w.dtype == torch.float32 and parent.dtype == torch.int32
    assert np.array_equal(parent.cpu().numpy(), p_want)
    assert np.array_equal(bits(w.cpu().numpy()), bits(w_want))
    if name == '1x1':
        assert w.flatten().tolist() == [0.0, float('inf')] and parent.flatten().tolist() == [0, -1]
    if name == 'strip':
        assert w[0, 0, :30].tolist() == [float(x) for x in range(30)] and torch.isinf(w[0, 0, 30:]).all()
        assert parent[0, 0, :30].tolist() == [0] * 30 and (parent[0, 0, 30:] == -1).all()
    if name == 'empty':
        assert (parent == 32 * 65 + 32).all()
    if name == 'u_shape':
        assert np.isinf(w_want[:, 20, 30]).all() and w_want[1, 5, 8] == 0 and (p_want[1] == 5 * 33 + 8).sum() > 1
    if name == 'random':
        assert max(len(REF.chain(p_want[0], (x, y))) for y in range(40) for x in range(40)) >= 8


@pytest.mark.parametrize('name', ['u_shape', 'empty', 'random', 'strip'])
def test_one_and_three_launches_are_one_and_three_steps(name):
    """from the start state, so nowhere near converged; a launch is one Jacobi step of the whole plane"""
    from piml_amd import ops_scenario
    blocked, goal = case(name)
    gb, gg = on_gpu(name)
    for launches in (1, 3):
        w, parent, steps = ops_scenario.nav_sight_relax(gb, gg, launches=launches)
        want = REF.steps(blocked, goal, launches, sight_of(name))
        assert steps == launches
        assert np.array_equal(parent.cpu().numpy(), want[1]), (name, launches)
        assert np.array_equal(bits(w.cpu().numpy()), bits(want[0])), (name, launches)
        assert not REF.same(want, fixed_point(name)[:2])         # still on its way
    w, parent, steps = ops_scenario.nav_sight_relax(gb, gg, launches=0)
    assert steps == 0 and REF.same((w.cpu().numpy(), parent.cpu().numpy()), REF.start(goal))


def test_u_wall_of_the_design():
    """the 33 x 33 U wall: 32 steps, 64 queued, the chain of (28, 16)"""
    from piml_amd import ops_scenario
    w_want, p_want, n = fixed_point('u_wall')
    assert n == 32 and REF.chain(p_want[0], (28, 16)) == [(21, 25), (9, 25), (9, 23), (16, 16)]
    gb, gg = on_gpu('u_wall')
    w, parent, steps = ops_scenario.nav_sight_relax(gb, gg)
    assert steps == 64 and np.array_equal(parent.cpu().numpy(), p_want) and np.array_equal(bits(w.cpu().numpy()), bits(w_want))
    assert REF.chain(parent.cpu().numpy()[0], (28, 16)) == [(21, 25), (9, 25), (9, 23), (16, 16)]


def test_captured_batch_equals_the_eager_batch():
    from piml_amd import _lib, hip_graphs_safe, ops_scenario
    from piml_amd.ops import _ptr, _stream
    assert hip_graphs_safe()
    blocked, goal = case('u_shape')
    gb, gg = on_gpu('u_shape')
    w0, p0 = (torch.from_numpy(x).to(DEV) for x in REF.start(goal))
    L = _lib.lib()
    B = ops_scenario.NAV_SIGHT_BATCH

    def state():
        return [w0.clone(), p0.clone(), torch.empty_like(w0), torch.empty_like(p0),
                torch.full((2, 34, 33, 8), -1, device=DEV, dtype=torch.int32), torch.zeros(2, device=DEV, dtype=torch.int32)]

    def batch(s):
        _lib.check(L.piml_nav_sight_relax(_ptr(gb), _ptr(gg), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), _ptr(s[3]), _ptr(s[4]), 2, 33, 34,
                                          B, _ptr(s[5]), _stream()), 'piml_nav_sight_relax')
    one = state()
    batch(one)
    batch(one)                                                   # 64 steps: past the fixed point (60)
    two = state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch(two)
    two[0].copy_(w0)
    two[1].copy_(p0)
    two[4].fill_(-1)
    two[5].zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    w_want, p_want, n = fixed_point('u_shape')
    assert B < n <= 2 * B
    assert torch.equal(one[0].view(torch.int32), two[0].view(torch.int32)) and torch.equal(one[1], two[1])
    assert one[5].tolist() == two[5].tolist() == [1, 1]
    assert np.array_equal(two[1].cpu().numpy(), p_want) and np.array_equal(bits(two[0].cpu().numpy()), bits(w_want))
    two[5].zero_()
    graph.replay()                                               # at the fixed point nothing changes
    torch.cuda.synchronize()
    assert two[5].tolist() == [0, 0] and torch.equal(one[0].view(torch.int32), two[0].view(torch.int32)) and torch.equal(one[1], two[1])


# ---- 2. the lookup ----

def lookup_inputs():
    from test_navfield_gpu import CELL, NEAR, X0, Y0, lookup_rows, lookup_want
    return (X0, Y0, CELL, NEAR), lookup_rows(), lookup_want()


@functools.lru_cache(maxsize=None)
def lookup_want_sight():
    (x0, y0, cell, near), (P, gate, dest), base = lookup_inputs()
    u = nav_ref.solve(*case('u_shape'))[0]
    return REF.direction(u, fixed_point('u_shape')[1], x0, y0, cell, near, P, gate, dest, base=base)


def lookup_fields():
    """(the U-shaped field with the table, the same field without)"""
    from piml_amd import ops_scenario
    (x0, y0, cell, near), _, _ = lookup_inputs()
    gb, gg = on_gpu('u_shape')
    u = torch.from_numpy(nav_ref.solve(*case('u_shape'))[0]).to(DEV)
    w, parent, _ = fixed_point('u_shape')
    with_ = ops_scenario.NavField(u, gb, gg, x0, y0, cell, near, w=torch.from_numpy(np.array(w)).to(DEV),
                                  parent=torch.from_numpy(np.array(parent)).to(DEV))
    return with_, ops_scenario.NavField(u, gb, gg, x0, y0, cell, near)


def test_lookup_matches_the_restatement():
    from piml_amd import ops_scenario
    (x0, y0, cell, near), (P, gate, dest), base = lookup_inputs()
    e_want, b_want, k_want = lookup_want_sight()
    with_, without = lookup_fields()
    tp, tg, td = (torch.from_numpy(x).to(DEV) for x in (P, gate, dest))
    e, b, k = ops_scenario.nav_direction(tp, tg, td, with_, return_branch=True)
    counts = np.bincount(b_want, minlength=4)
    print(f'\n[navsight] lookup: {len(P)} rows, branches {counts.tolist()} (without the table {np.bincount(base[1], minlength=4).tolist()})')
    b, k, e = b.cpu().numpy(), k.cpu().numpy(), e.cpu().numpy().astype(np.float64)
    assert np.array_equal(b, b_want), np.flatnonzero(b != b_want)[:10]
    assert np.array_equal(k, k_want), np.flatnonzero(k != k_want)[:10]
    fin = np.isfinite(e_want).all(1)
    assert np.array_equal(np.isfinite(e).all(1), fin)
    err = np.abs(e[fin] - e_want[fin]).max()
    print(f'[navsight] lookup: largest direction error {err:.3g}')
    assert err <= 1e-5
    # where the field applies the table takes every row (each reachable cell beyond near has a parent); elsewhere nothing moved
    assert len(P) > 3000 and counts[3] > 1000 and counts[0] > 500
    assert np.array_equal(b_want == 3, base[1] > 0) and (k_want[b_want == 3] == -1).all()
    assert np.array_equal(bits(e[b_want == 0].astype(f32)), bits(ops_scenario.nav_direction(tp, tg, td, without).cpu().numpy()[b_want == 0]))
    # forced off, the lookup is piml_nav_direction's bit for bit
    off = ops_scenario.nav_direction(tp, tg, td, with_, return_branch=True, sight=False)
    old = ops_scenario.nav_direction(tp, tg, td, without, return_branch=True)
    assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(off, old))
    assert np.array_equal(old[1].cpu().numpy(), base[1]) and int((old[1] == 3).sum()) == 0
    on = ops_scenario.nav_direction(tp, tg, td, with_, return_branch=True, sight=True)
    assert np.array_equal(on[1].cpu().numpy(), b_want)
    with pytest.raises(ValueError, match='sight=True'):
        ops_scenario.nav_direction(tp, tg, td, without, sight=True)
    empty = ops_scenario.nav_direction(tp[:0], tg[:0], td[:0], with_, return_branch=True)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    # a parent that is the cell itself, or -1, leaves the row to the other branches
    own = with_.parent.clone()
    lin = torch.arange(33 * 34, device=DEV, dtype=torch.int32).reshape(1, 34, 33)
    own[0] = lin[0]
    own[1] = -1
    from piml_amd import ops_scenario as O
    inert = O.NavField(with_.u, with_.blocked, with_.goal, x0, y0, cell, near, parent=own)
    got = O.nav_direction(tp, tg, td, inert, return_branch=True)
    assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(got, old))


# ---- 3. the frame ----

SEEDS = [0, 1, 2]
PLAIN = dict(version='GC', **LAW)
WALLED = dict(PLAIN, Aw=50.0, Bw=-5.0)
NOISY = dict(WALLED, An=0.5, noise_tau=0.5)
# two rooms and a door, as in test_scenario_nav_gpu.py: gates at x = 0 and x = 10 over y in [0.5, 3]; a wall on x = 5 from below
# the grid to above it, open over y in (4.5, 5.5)
WALLS = [[[5.0, -2.0], [5.0, 4.5]], [[5.0, 5.5], [5.0, 9.5]]]
GATES = [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]
BOUNDS = (-1.5, -1.0, 11.5, 8.0)
CAP = 64


def MLAPM(**params):
    from piml_amd.models.mlapm import MLAPM as M
    return M(**params)


@functools.lru_cache(maxsize=None)
def scene(name):
    from piml_amd import scenarios
    if name == 'gc':
        return dataclasses.replace(scenarios.gc_scenario(), route_max_iters=0).to(DEV)
    if name == 'open':                                           # one room: its long sides, the two gates, nothing between them
        sides = [[[-1.0, -0.5], [11.0, -0.5]], [[-1.0, 7.5], [11.0, 7.5]]]
        return scenarios.floorplan_scenario(sides, GATES, n_initial=10, rate_per_s=1.2).to(DEV)
    kw = dict(n_initial=12, rate_per_s=2.0, arrival_radius=0.5) if name == 'plan' else dict(n_initial=10, rate_per_s=1.2)
    return scenarios.floorplan_scenario(WALLS, GATES, **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def field(name, sight=True):
    """the scene's field with the table; sight = False: the same field without; 'gc-inert': GC's field with a table of -1"""
    from piml_amd import ops_scenario
    if name == 'gc-inert':
        f = field('gc', False)
        return ops_scenario.NavField(f.u, f.blocked, f.goal, f.x0, f.y0, f.cell, f.near, f.clearance, f.iterations,
                                     parent=torch.full_like(f.u, -1, dtype=torch.int32))
    if name == 'gc':
        return ops_scenario.nav_field(scene('gc'), cell=0.5, clearance=0.3, device=DEV, sight=sight)
    return ops_scenario.nav_field(scene(name), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV, sight=sight)


def test_field_with_the_table_is_the_field_and_the_restatement():
    f, g = field('plan'), field('plan', False)
    assert torch.equal(f.u.view(torch.int32), g.u.view(torch.int32)) and torch.equal(f.blocked, g.blocked)
    assert g.parent is None and g.sight_desc is None and f.sight_desc is not None and f.iterations == g.iterations
    got = f.to_numpy()
    w, parent, n = REF.solve(got.blocked, got.goal)
    print(f'\n[navsight] two rooms: {got.gx} x {got.gy} cells, fixed point after {n} steps, {f.sight_iterations} queued '
          f'(first-order field: {f.iterations})')
    assert np.array_equal(got.parent, parent) and np.array_equal(bits(got.w), bits(w)) and f.sight_iterations >= n
    assert np.array_equal(np.isfinite(got.w), np.isfinite(got.u))


@pytest.mark.parametrize('params', [PLAIN, WALLED, NOISY], ids=['plain', 'walls', 'walls+noise'])
def test_table_of_minus_one_is_the_nav_frame(params):
    """single, members and table forms on GC over 40 frames: with no parent anywhere branch 3 never applies"""
    sc, inert, nav = scene('gc'), field('gc-inert'), field('gc', False)
    sim = MLAPM(**params)
    want = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=nav)
    straight = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP)
    assert sum(want.spawned) > 3 * 20 and not _same(want.member(0), straight.member(0))        # the field routes
    got = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=inert)
    assert all(_same(got.member(m), want.member(m)) for m in range(len(SEEDS)))
    assert _same(sim.simulate_scenario(sc, 40, seed=SEEDS[1], capacity=CAP, nav=inert), want.member(1))
    table = sim.simulate_sweep(sc, 40, [params], SEEDS, capacity=CAP, nav=inert)
    assert all(_same(table.member(m), want.member(m)) for m in range(len(SEEDS)))
    real = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=field('gc'))
    assert not _same(real.member(0), want.member(0))             # and GC's own table does move them


def _first_frame(params, nav, overwrite=None):
    """the state after the init launch and ONE frame of the plan under `params`; overwrite(st): edits the state in between"""
    from piml_amd import ops_scenario, scenarios
    from piml_amd.models import mlapm
    sim = MLAPM(**params)
    st = scenarios.scenario_state_for(scene('plan'), 3, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step_mlapm(st, None, init=True)
    if overwrite is not None:
        overwrite(st)
    wall, noise = mlapm.wall_args(params), mlapm.noise_args(params)
    walls = None if wall is None else (ops_scenario.wall_grid(st.scenario.obstacles, wall[2], DEV), ops_scenario.wall_law(*wall[:2]))
    ops_scenario.scenario_step_mlapm(st, sim._law(0.3), walls=walls, nav=nav,
                                     noise=None if noise is None else ops_scenario.noise_law(*noise, float(st.scenario.time_unit)))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize('params', [PLAIN, NOISY], ids=['plain', 'walls+noise'])
def test_first_frame_is_the_plain_frame_steered_to_p_plus_e(params):
    """v', a' and p' of the frame with the table == the plain frame's on a state whose destination is p + e of
    nav_direction(..., field) where the branch is > 0, bitwise, for the agents that arrived nowhere"""
    from piml_amd import ops_scenario
    nav = field('plan')
    seen = {}

    def overwrite(st):
        gate = torch.gather(st.exit_idx, 1, st.flag.long().unsqueeze(1)).squeeze(1)
        e, b, _ = ops_scenario.nav_direction(st.p, gate, st.dest, nav, return_branch=True)
        seen.update(p=st.p.clone(), b=b, present=st.mask == 1)
        st.dest.copy_(torch.where((b > 0).unsqueeze(-1), st.p + e, st.dest))
    got = _first_frame(params, nav)
    want = _first_frame(params, None, overwrite)
    first_order = _first_frame(params, field('plan', False))
    stayed = seen['present'] & (got.mask == 1) & (want.mask == 1) & (got.flag == 0) & (want.flag == 0)
    routed = stayed & (seen['b'] == 3)
    print(f'\n[navsight] first frame: {int(seen["present"].sum())} agents, {int(stayed.sum())} arrived nowhere, branches '
          f'{torch.bincount(seen["b"][seen["present"]].long(), minlength=4).tolist()}')
    assert int(seen['present'].sum()) == 3 * 12 and int(routed.sum()) >= 24 and int((seen['b'][seen['present']] == 1).sum()) == 0
    for k in ('v', 'a', 'p'):
        assert torch.equal(tbits(getattr(got, k)[stayed]), tbits(getattr(want, k)[stayed])), k
    assert not torch.equal(tbits(got.v[routed]), tbits(first_order.v[routed]))   # the table moved e off the gradient
    assert torch.equal(tbits(got.v[stayed & ~routed]), tbits(first_order.v[stayed & ~routed]))


@functools.lru_cache(maxsize=None)
def plan_runs(kind):
    sim = MLAPM(**WALLED)
    nav = {'none': None, 'nav': field('plan', False), 'sight': field('plan')}[kind]
    return sim.simulate_ensemble(scene('plan'), 60, SEEDS, capacity=CAP, nav=nav)


def test_arrivals_do_not_depend_on_the_table():
    plain, routed = plan_runs('none'), plan_runs('sight')
    assert routed.spawned == plain.spawned and routed.dropped == plain.dropped and sum(plain.spawned) > 3 * 12
    for k in ('spawn_count', 'desired_speed', 'waypoints'):
        assert torch.equal(tbits(getattr(routed, k)), tbits(getattr(plain, k))), k
    assert torch.equal(routed.state.exit_idx, plain.state.exit_idx)
    born = torch.zeros_like(plain.mask_p, dtype=torch.bool)
    born[:, 0] = plain.mask_p[:, 0] == 1
    born[:, 1:] = (plain.mask_p[:, 1:] == 1) & (plain.mask_p[:, :-1] == 0)
    assert torch.equal(tbits(routed.position[born]), tbits(plain.position[born]))
    assert not torch.equal(tbits(routed.position), tbits(plain.position))
    assert not torch.equal(tbits(routed.position), tbits(plan_runs('nav').position))


def test_members_table_forms_and_captured_replay_are_bitwise_equal():
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    sc, nav, ens = scene('plan'), field('plan'), plan_runs('sight')
    for params, base in ((WALLED, ens), (NOISY, None), (PLAIN, None)):
        sim = MLAPM(**params)
        base = base or sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav)
        for m, s in enumerate(SEEDS):                             # member m of an ensemble is the single run
            assert _same(base.member(m), sim.simulate_scenario(sc, 60, seed=s, capacity=CAP, nav=nav)), (m, params)
        table = sim.simulate_sweep(sc, 60, [params], SEEDS, capacity=CAP, nav=nav)          # law, wall and noise tables
        graph = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav, use_graph=True)
        eager = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav, use_graph=False)
        for m in range(len(SEEDS)):
            assert _same(table.member(m), base.member(m)) and _same(graph.member(m), eager.member(m)), (m, params)
            assert _same(graph.member(m), base.member(m))


def _crossings(res):
    """(y of every recorded step across x = 5, how many agents took one)"""
    p, m = res.position.cpu().numpy().astype(np.float64), res.mask_p.cpu().numpy()
    a, b = p[:, :-1], p[:, 1:]
    both = (m[:, :-1] == 1) & (m[:, 1:] == 1)
    with np.errstate(invalid='ignore'):
        hit = both & ((a[..., 0] - 5.0) * (b[..., 0] - 5.0) < 0)
    w = (5.0 - a[..., 0][hit]) / (b[..., 0][hit] - a[..., 0][hit])
    return a[..., 1][hit] + w * (b[..., 1][hit] - a[..., 1][hit]), int(hit.any(1).sum())


def test_two_rooms_and_a_door():
    """pair forces off (A = 0), 400 frames, 2 seeds: every recorded step across x = 5 lies in the door, every agent of the
    first 100 frames has retired, and no recorded position lies in a blocked cell of the field"""
    law = dict(PLAIN, A=0.0, tau=0.5)
    sc, nav = scene('rooms'), field('rooms')
    routed = MLAPM(**law).simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP, nav=nav)
    assert routed.dropped == [0, 0] and min(routed.spawned) >= 30
    y, agents = _crossings(routed)
    print(f'\n[navsight] two rooms: {y.size} steps across x = 5 by {agents} agents, y in [{y.min():.3f}, {y.max():.3f}]')
    assert y.size >= 40 and ((y > 4.5) & (y < 5.5)).all()
    m = routed.mask_p.cpu().numpy()
    early = (m[:, :100] == 1).any(1)
    assert early.sum() >= 2 * 12 and (m[:, -1][early] == 0).all()
    pos = routed.position.cpu().numpy()[m == 1]
    cx = np.floor((pos[:, 0] - f32(nav.x0)) / f32(nav.cell)).astype(int)
    cy = np.floor((pos[:, 1] - f32(nav.y0)) / f32(nav.cell)).astype(int)
    inside = (cx >= 0) & (cx < nav.gx) & (cy >= 0) & (cy < nav.gy)
    blocked = nav.blocked.cpu().numpy()
    n_in = int(blocked[cy[inside], cx[inside]].sum())
    print(f'[navsight] two rooms: {len(pos)} recorded positions, {int((~inside).sum())} outside the grid, {n_in} in a blocked cell')
    assert inside.sum() > 0.9 * len(pos) and n_in == 0


def test_open_room_tracks_are_no_less_straight():
    """one room, two gates, no inner wall, A = 0: the mean straightness (net displacement / path length) of the tracks that
    retire, with the table against the first-order field"""
    law = dict(PLAIN, A=0.0, tau=0.5)
    sc = scene('open')
    runs = {k: MLAPM(**law).simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP, nav=field('open', k == 'sight'))
            for k in ('nav', 'sight')}
    stats = {k: r.track_stats() for k, r in runs.items()}
    s = {k: v.mean_straightness('complete') for k, v in stats.items()}
    done = {k: v.summary()['complete_tracks'] for k, v in stats.items()}
    print(f'\n[navsight] open room: mean straightness of the tracks that retire {s["sight"]:.5f} with the table ({done["sight"]} tracks), '
          f'{s["nav"]:.5f} with the first-order field ({done["nav"]} tracks)')
    assert min(done.values()) >= 40
    assert s['sight'] >= s['nav']


def test_errors_and_the_command_line(tmp_path):
    from piml_amd import _lib, ops_scenario, scenarios
    sc, nav = scene('plan'), field('plan')
    law = ops_scenario.mlapm_law()
    st = scenarios.scenario_state_for(scene('gc'), 4, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st, init=True)
    with pytest.raises(ValueError, match='gates'):
        ops_scenario.scenario_step_mlapm(st, law, nav=nav)       # 2 gates for a scene of 7
    # the entry's own refusals, with descriptors that pass but for the one thing
    gc = field('gc-inert')
    call = lambda s, navd, sd: _lib.lib().piml_scenario_step_mlapm_sight(
        ctypes.byref(s), ctypes.byref(st.rules), 3, st.seeds.data_ptr(), ctypes.byref(law), None, None, None, None,
        ctypes.byref(navd), None if sd is None else ctypes.byref(sd), None, 0, None)
    iters = _lib.Scenario.from_buffer_copy(st.desc)
    iters.route_max_iters = 1
    wrong = _lib.NavGrid.from_buffer_copy(gc.desc)
    wrong.G = 6
    assert call(iters, gc.desc, gc.sight_desc) == 1 and call(st.desc, wrong, gc.sight_desc) == 1
    assert call(st.desc, gc.desc, None) == 1
    for name, value in (('parent', None), ('G', 6), ('gx', gc.gx + 1), ('gy', gc.gy - 1)):
        bad = _lib.NavSight.from_buffer_copy(gc.sight_desc)
        setattr(bad, name, value)
        assert call(st.desc, gc.desc, bad) == 1, name
    assert int(st.t.item()) == 0
    assert call(st.desc, gc.desc, gc.sight_desc) == 0            # the argument set every refusal differs from
    torch.cuda.synchronize()
    # nav='sight' builds the scene's field with the defaults and the table; True stays the first-order field
    auto = MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav='sight')
    default = ops_scenario.nav_field(sc, device=DEV, sight=True)
    assert _same(auto, MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=default))
    plain = MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=True)
    assert _same(plain, MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=ops_scenario.nav_field(sc, device=DEV)))
    assert not _same(auto, plain)
    # the command line on a plan file
    plan = tmp_path / 'plan.json'
    plan.write_text(json.dumps(dict(walls=WALLS, gates=GATES, n_initial=12, rate_per_s=2.0, arrival_radius=0.5)))
    out = tmp_path / 'walls.json'
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scene-plan', str(plan), '--nav',
                        '--nav-sight', '--frames', '60', '--seeds', '0:2', '--capacity', str(CAP), '--obstacle-stats', str(out)],
                       cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'floor field: 2 gates' in p.stdout and f'lines of sight: {default.sight_iterations} steps' in p.stdout
    from piml_amd.obstaclestats import ADDITIVE, ObstacleStats
    got = ObstacleStats.from_json(str(out))
    want = MLAPM(**PLAIN).simulate_ensemble(sc, 60, [0, 1], capacity=CAP, nav=default).obstacle_stats()
    assert all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ADDITIVE)
    first = MLAPM(**PLAIN).simulate_ensemble(sc, 60, [0, 1], capacity=CAP, nav=True).obstacle_stats()
    assert not all(np.array_equal(getattr(first, k), getattr(want, k)) for k in ADDITIVE)       # the table ran
