"""GPU: the density-aware floor field (piml_nav_density, piml_nav_cost, piml_nav_relax_cost, piml_scenario_step_mlapm_navdyn;
MLAPM.simulate_*(..., nav_density=)).  The deposit is the restatement's integers, the cost and the solve its bits
(tests/navcost_ref.py), before convergence as well; cost == 1 is piml_nav_relax; the chain on the two-door plan sends the
prototype's probes to the prototype's doors; a run with kd = 0 is the run with the static field, members and captured replays
are bitwise each other, stride 0 is piml_scenario_step_mlapm_nav; and in two rooms joined by two doors a crowd that queues at
the near door starts to use the far one."""
import functools

import numpy as np
import pytest
import torch

import nav_ref
import navcost_ref as REF
from test_scenario_mlapm_gpu import LAW, _same, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = [0, 1, 2]
PLAIN = dict(version='GC', **LAW)
WALLED = dict(PLAIN, Aw=50.0, Bw=-5.0)
f32 = np.float32
NAN = float('nan')
GRIDS = [(1, 1), (40, 1), (33, 34), (65, 65)]                    # (gx, gy): one cell, one row, across a tile edge, three tiles


def MLAPM(**params):
    from piml_amd.models.mlapm import MLAPM as M
    return M(**params)


def grid_field(gx, gy, x0=0.0, y0=0.0, cell=0.5, blocked=None, goal=None, near=0.0):
    """a NavField over a grid that was not solved: the operators read its scalars, blocked and goal only"""
    from piml_amd import ops_scenario
    blocked = np.zeros((gy, gx), np.uint8) if blocked is None else blocked
    goal = np.zeros((1, gy, gx), np.uint8) if goal is None else goal
    u = torch.full(goal.shape, float('inf'), device=DEV)
    return ops_scenario.NavField(u, torch.from_numpy(blocked).to(DEV), torch.from_numpy(goal).to(DEV), x0, y0, cell, near)


def u32(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, f32).view(np.uint32)


# ---- 1. the deposit ----

@pytest.mark.parametrize('members', [1, 3])
@pytest.mark.parametrize('cap', [1, 65, 300])
def test_deposit_is_the_restatement(cap, members):
    """7 x 5 cells of 0.25 from (-1, 2): agents on cell boundaries, on the outer edges, outside, NaN and absent"""
    from piml_amd import ops_scenario
    gx, gy, x0, y0, cell = 7, 5, -1.0, 2.0, 0.25
    rng = np.random.default_rng(100 * cap + members)
    P = np.stack([rng.uniform(x0 - 0.5, x0 + gx * cell + 0.5, (members, cap)),
                  rng.uniform(y0 - 0.5, y0 + gy * cell + 0.5, (members, cap))], -1).astype(f32)
    special = [(x0, y0), (x0 + gx * cell, y0 + 0.1), (x0 + 0.1, y0 + gy * cell), (x0 + 3 * cell, y0 + 2 * cell), (NAN, y0 + 0.1),
               (x0 + 0.1, NAN), (np.nextafter(f32(x0), f32(-9)), y0 + 0.1), (x0 + 0.1, np.nextafter(f32(y0 + gy * cell), f32(0))),
               (1e30, y0), (x0 - 100.0, y0 + 0.1), (float('inf'), y0 + 0.1), (x0 + 5 * cell, y0 + 4 * cell)]
    for m in range(members):
        for k, q in enumerate(special[m:]):                      # (capacity 1: member m gets special case m)
            if k < cap:
                P[m, k] = q
    mask = (rng.uniform(size=(members, cap)) < 0.8).astype(f32)
    mask[:, :min(cap, 4)] = 1
    field = grid_field(gx, gy, x0, y0, cell)
    want = REF.deposit(P, mask, x0, y0, cell, gx, gy)
    pos, msk = torch.from_numpy(P).to(DEV), torch.from_numpy(mask).to(DEV)
    got = ops_scenario.nav_density(pos, msk, field)
    assert got.dtype == torch.int32 and tuple(got.shape) == (members, gy, gx)
    assert np.array_equal(got.cpu().numpy(), want)
    if cap > 1:
        assert 0 < want.sum() < mask.sum()                       # some are inside, some present ones are not
    dirty = torch.full_like(got, 7)                              # a second call on a dirty count: the entry zeroes it
    assert ops_scenario.nav_density(pos, msk, field, out=dirty) is dirty and torch.equal(dirty, got)
    if members == 1:                                             # a single run's state has no member axis
        assert torch.equal(ops_scenario.nav_density(pos[0], msk[0], field), got)


def test_deposit_of_300_agents_in_one_cell():
    from piml_amd import ops_scenario
    field = grid_field(7, 5, -1.0, 2.0, 0.25)
    P = np.empty((2, 300, 2), f32)
    P[0] = (-1.0 + 2.5 * 0.25, 2.0 + 3.5 * 0.25)
    P[1] = (-1.0 + 6.9 * 0.25, 2.0 + 0.1 * 0.25)
    got = ops_scenario.nav_density(torch.from_numpy(P).to(DEV), torch.ones(2, 300, device=DEV), field).cpu().numpy()
    want = np.zeros((2, 5, 7), np.int32)
    want[0, 3, 2], want[1, 0, 6] = 300, 300
    assert np.array_equal(got, want)                             # integer atomics: exact, and no member touches another's plane


# ---- 2. the cost ----

@pytest.mark.parametrize('r', [0, 1, 4, 8])
@pytest.mark.parametrize('gx,gy', GRIDS)
def test_cost_is_the_restatement(gx, gy, r):
    from piml_amd import ops_scenario
    cell = 0.5
    rng = np.random.default_rng(1000 * gx + 10 * gy + r)
    count = rng.integers(0, 4, (2, gy, gx)).astype(np.int32)
    count[1] = (rng.uniform(size=(gy, gx)) < 0.1) * rng.integers(1, 30, (gy, gx))
    field = grid_field(gx, gy, cell=cell)
    law = ops_scenario.nav_density_law(2.0, rho0=0.5, radius=r * cell, fmax=8.0)
    assert law.radius_cells(cell) == r
    want, rho = REF.cost(count, cell, r, 2.0, 0.5, 8.0)
    got = ops_scenario.nav_cost(torch.from_numpy(count).to(DEV), field, law)
    assert np.array_equal(u32(got), u32(want))
    if gx * gy > 1:
        assert want.min() >= 1.0 and want.max() <= 8.0 and (rho > 0.5).any()
    zero = ops_scenario.nav_cost(torch.from_numpy(count).to(DEV), field, ops_scenario.nav_density_law(0.0, radius=r * cell))
    assert (zero == 1.0).all()                                   # kd = 0


def test_cost_at_rho0_and_at_fmax():
    from piml_amd import ops_scenario
    count = np.zeros((1, 4, 5), np.int32)
    count[0, 1, 1], count[0, 3, 4] = 9, 200
    field = grid_field(5, 4, cell=1.0)
    dev = torch.from_numpy(count).to(DEV)
    law = ops_scenario.nav_density_law(2.0, rho0=1.0, radius=1.0, fmax=8.0)           # 9 agents over 9 m^2: rho == rho0 exactly
    want, rho = REF.cost(count, 1.0, 1, 2.0, 1.0, 8.0)
    got = ops_scenario.nav_cost(dev, field, law)
    assert rho[0, 1, 1] == 1.0 and want[0, 1, 1] == 1.0 and want[0, 3, 4] == 8.0 and rho[0, 3, 4] > 20
    assert np.array_equal(u32(got), u32(want))
    sharp = ops_scenario.nav_cost(dev, field, ops_scenario.nav_density_law(2.0, rho0=9.0, radius=0.0, fmax=1.0))
    assert (sharp == 1.0).all()                                  # fmax = 1 clips everything


# ---- 3. the solve ----

@functools.lru_cache(maxsize=None)
def solve_case(gx, gy):
    """blocked (gy, gx), goal (2, gy, gx), cost (3, gy, gx) in [1, 4] -- a different plane per member -- and the restatement's
    fixed points (3, 2, gy, gx) with their step counts, computed once"""
    rng = np.random.default_rng(gx * 100 + gy)
    if (gx, gy) == (33, 34):
        blocked, goal = nav_ref.u_shape_case()
    else:
        blocked = (rng.uniform(size=(gy, gx)) < 0.15).astype(np.uint8)
        goal = np.zeros((2, gy, gx), np.uint8)
        goal[0, gy // 2, gx // 2] = 1
        goal[1, 0, 0] = 1
        goal[1, gy - 1, gx - 1] = 1
    cost = rng.uniform(1, 4, (3, gy, gx)).astype(f32)
    cost[2] = 1.0 + 7.0 * (rng.uniform(size=(gy, gx)) < 0.2)     # member 2: plateaus of 8 in a field of 1
    solved = [REF.solve(blocked, goal, cost[m]) for m in range(3)]
    return blocked, goal, cost, np.stack([u for u, _ in solved]), [n for _, n in solved]


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


@pytest.mark.parametrize('gx,gy', GRIDS)
def test_solve_is_the_restatement(gx, gy):
    """three members with different cost planes and two gates: a cost indexed by plane instead of by member would show"""
    from piml_amd import ops_scenario
    blocked, goal, cost, want, n = solve_case(gx, gy)
    b, g, c = dev(blocked, goal, cost)
    u, steps = ops_scenario.nav_relax_cost(b, g, c)
    assert tuple(u.shape) == (3, 2, gy, gx) and steps % 128 == 0 and steps >= max(n)
    assert np.array_equal(u32(u), u32(want))
    if gx * gy > 40:
        assert not np.array_equal(u32(want[0]), u32(want[1]))    # the members do differ
    one, _ = ops_scenario.nav_relax_cost(b, g, c[1:2])           # a single member is that member's planes
    assert np.array_equal(u32(one[0]), u32(want[1]))


@pytest.mark.parametrize('launches', [1, 3])
def test_solve_before_convergence_is_exact(launches):
    """K = 8 steps per launch on tiles with a halo of 8: bitwise 8 and 24 steps of the whole plane from the cold start"""
    from piml_amd import ops_scenario
    for gx, gy in ((33, 34), (65, 65)):
        blocked, goal, cost, _, n = solve_case(gx, gy)
        assert min(n) > 8 * launches                             # not yet converged
        b, g, c = dev(blocked, goal, cost)
        u, steps = ops_scenario.nav_relax_cost(b, g, c, launches=launches)
        assert steps == 8 * launches
        for m in range(3):
            want = REF.steps(nav_ref.start(goal), blocked, goal, cost[m], 8 * launches)
            assert np.array_equal(u32(u[m]), u32(want)), (gx, gy, m)


def test_unit_cost_is_nav_relax_bit_for_bit():
    from piml_amd import ops_scenario
    for gx, gy in ((33, 34), (65, 65)):
        blocked, goal = solve_case(gx, gy)[:2]
        b, g = dev(blocked, goal)
        ones = torch.ones(2, gy, gx, device=DEV)
        for launches in (1, 3, None):
            want, n0 = ops_scenario.nav_relax(b, g, launches=launches)
            got, n1 = ops_scenario.nav_relax_cost(b, g, ones, launches=launches)
            assert n0 == n1 and torch.equal(bits(got[0]), bits(want)) and torch.equal(bits(got[1]), bits(want)), (gx, launches)


def test_a_captured_batch_is_the_eager_one():
    from piml_amd import _lib, hip_graphs_safe
    assert hip_graphs_safe()
    blocked, goal, cost, want, n = solve_case(33, 34)
    b, g, c = dev(blocked, goal, cost)
    start = torch.from_numpy(nav_ref.start(goal)).to(DEV).unsqueeze(0).repeat(3, 1, 1, 1).contiguous()
    ua, ub = start.clone(), torch.empty_like(start)
    changed = torch.zeros(6, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _lib.check(_lib.lib().piml_nav_relax_cost(b.data_ptr(), g.data_ptr(), c.data_ptr(), ua.data_ptr(), ub.data_ptr(), 3, 2,
                                                      33, 34, 16, changed.data_ptr(), stream.cuda_stream), 'piml_nav_relax_cost')
        graph.replay()
    torch.cuda.synchronize()
    assert max(n) <= 128 and np.array_equal(u32(ua), u32(want)) and changed.tolist() == [1] * 6
    changed.zero_()
    with torch.cuda.stream(stream):
        graph.replay()                                           # from the fixed point: nothing changes
    torch.cuda.synchronize()
    assert np.array_equal(u32(ua), u32(want)) and changed.tolist() == [0] * 6


# ---- 4. the chain on the device: two rooms, two doors ----

def test_chain_sends_the_probes_to_the_prototypes_doors():
    """positions placed by hand -> density -> cost -> solve, each the restatement's bits, -> nav_direction over the member's
    plane: every probe walks down its member's field in steps of half a cell until it stands on the wall's column"""
    from piml_amd import ops_scenario
    blocked, goal, count = REF.two_door_case()
    base = grid_field(40, 24, 0.0, 0.0, REF.TWO_DOOR_CELL, blocked, goal)
    dyn = ops_scenario.NavFieldDynamic(base, 2)
    P = np.full((2, 32, 2), NAN, f32)
    P[:, :25] = REF.two_door_positions()
    mask = np.zeros((2, 32), f32)
    mask[:, :25] = 1
    P[1, 30], mask[1, 30] = (3.3, 3.3), 0                        # an absent slot with a position: not counted
    st = type('State', (), dict(p=torch.from_numpy(P).to(DEV), mask=torch.from_numpy(mask).to(DEV),
                                seeds=torch.zeros(2, dtype=torch.long, device=DEV)))()
    want_doors = {0.0: [True] * 7, 2.0: [False, False, False, False, False, True, False]}
    for kd, at_near in want_doors.items():
        law = ops_scenario.nav_density_law(kd, rho0=0.5, radius=0.5, fmax=8.0)     # r = 1 cell
        steps = ops_scenario.nav_field_update(dyn, st, law)
        f, _ = REF.cost(count, REF.TWO_DOOR_CELL, 1, kd, 0.5, 8.0)
        u, n = REF.solve(blocked, goal, f)
        assert n == (63 if kd else 58) and steps == 256 and dyn.iterations == 256         # a batch that changes, one that does not
        for m in range(2):
            assert np.array_equal(dyn.count[m].cpu().numpy(), count)
            assert np.array_equal(u32(dyn.cost[m]), u32(f)) and np.array_equal(u32(dyn.u[m]), u32(u))
        plane = dyn.member(1)
        p = torch.tensor([[(x + 0.5) * 0.5, (y + 0.5) * 0.5] for x, y in REF.TWO_DOOR_PROBES], device=DEV)
        gate = torch.zeros(7, dtype=torch.int32, device=DEV)
        dest = torch.tensor([[18.25, 2.75]], device=DEV).repeat(7, 1)
        rows = torch.full((7,), -1, dtype=torch.long, device=DEV)
        for _ in range(200):
            p = p + 0.25 * ops_scenario.nav_direction(p, gate, dest, plane)
            on_wall = (torch.floor(p[:, 0] / 0.5) >= REF.TWO_DOOR_WALL) & (rows < 0)
            rows = torch.where(on_wall, torch.floor(p[:, 1] / 0.5).long(), rows)
        rows = rows.tolist()
        assert [r in REF.NEAR_DOOR for r in rows] == at_near, (kd, rows)
        assert all(r in REF.NEAR_DOOR + REF.FAR_DOOR for r in rows), (kd, rows)


# ---- 5. the frame ----
# test_scenario_nav_gpu.py's plan: two rooms and one door, 12 initial agents, 2 arrivals a second
WALLS = [[[5.0, -2.0], [5.0, 4.5]], [[5.0, 5.5], [5.0, 9.5]]]
GATES = [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]
BOUNDS = (-1.5, -1.0, 11.5, 8.0)
CAP = 64
FRAMES = 60                                                      # updates before frames 1, 9, 17, ..., 57: eight of them


@functools.lru_cache(maxsize=None)
def scene():
    from piml_amd import scenarios
    return scenarios.floorplan_scenario(WALLS, GATES, n_initial=12, rate_per_s=2.0, arrival_radius=0.5).to(DEV)


@functools.lru_cache(maxsize=None)
def field():
    from piml_amd import ops_scenario
    return ops_scenario.nav_field(scene(), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV)


def density(kd, **kw):
    from piml_amd import ops_scenario
    return ops_scenario.nav_density_law(kd, **kw)


@functools.lru_cache(maxsize=None)
def static_run():
    return MLAPM(**WALLED).simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field())


@functools.lru_cache(maxsize=None)
def dense_run():
    """rho0 = 0: every agent raises the cost around it, so the fields differ from the static one from the first update"""
    return MLAPM(**WALLED).simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(4.0, rho0=0.0))


def test_kd_zero_is_the_run_with_the_static_field():
    """eight cold-start solves per member, each landing on the static field's bits; single, members and table forms"""
    sim, law = MLAPM(**WALLED), density(0.0)
    got = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=law)
    assert all(_same(got.member(m), static_run().member(m)) for m in range(3))
    one = sim.simulate_scenario(scene(), FRAMES, seed=SEEDS[1], capacity=CAP, nav=field(), nav_density=law)
    assert _same(one, static_run().member(1))
    table = sim.simulate_sweep(scene(), FRAMES, [WALLED], SEEDS, capacity=CAP, nav=field(), nav_density=law)
    assert all(_same(table.member(m), static_run().member(m)) for m in range(3))
    auto = sim.simulate_scenario(scene(), 20, seed=1, capacity=CAP, nav=True, nav_density=law)      # nav=True builds the field
    assert _same(auto, sim.simulate_scenario(scene(), 20, seed=1, capacity=CAP, nav=True))


def test_the_density_term_moves_the_run_and_members_are_single_runs():
    sim, law = MLAPM(**WALLED), density(4.0, rho0=0.0)
    ens = dense_run()
    assert ens.spawned == static_run().spawned                   # the arrivals do not depend on the field
    for m, s in enumerate(SEEDS):
        assert not _same(ens.member(m), static_run().member(m))  # the term acts ...
        one = sim.simulate_scenario(scene(), FRAMES, seed=s, capacity=CAP, nav=field(), nav_density=law)
        assert _same(ens.member(m), one), m                      # ... per member: member m is the single run of its seed
    assert not torch.equal(bits(ens.position[0]), bits(ens.position[1]))
    table = sim.simulate_sweep(scene(), FRAMES, [WALLED], SEEDS, capacity=CAP, nav=field(), nav_density=law)
    assert all(_same(table.member(m), ens.member(m)) for m in range(3))


def test_a_captured_run_is_the_eager_one():
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    sim, law = MLAPM(**WALLED), density(4.0, rho0=0.0)
    graph = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=law, use_graph=True)
    eager = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=law, use_graph=False)
    assert all(_same(graph.member(m), eager.member(m)) and _same(graph.member(m), dense_run().member(m)) for m in range(3))
    wide = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(4.0, rho0=0.0, every=16),
                                 use_graph=True)
    assert not _same(wide.member(0), graph.member(0))            # (another schedule is another run)
    with pytest.raises(ValueError, match='multiple of frames_per_graph'):
        sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(4.0, every=12), use_graph=True)
    twelve = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(4.0, rho0=0.0, every=12),
                                   use_graph=True, frames_per_graph=4)
    assert _same(twelve.member(2), sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), use_graph=False,
                                                         nav_density=density(4.0, rho0=0.0, every=12)).member(2))


def test_stride_zero_is_the_static_frame():
    """the new entry with member_stride = 0 reads member 0's planes for every member: bitwise piml_scenario_step_mlapm_nav"""
    from piml_amd import ops_scenario, scenarios
    from piml_amd.models import mlapm
    dyn = ops_scenario.NavFieldDynamic(field(), 3)
    assert dyn.member_stride == dyn.G * dyn.gy * dyn.gx and torch.equal(bits(dyn.u[2]), bits(field().u))
    dyn.u[1:].fill_(float('inf'))                                # what a non-zero stride would read
    dyn.member_stride = 0
    sim = MLAPM(**WALLED)
    wall = mlapm.wall_args(WALLED)
    runs = []
    for nav in (dyn, field()):
        st = scenarios.scenario_state_for(scene(), FRAMES, CAP, DEV, seeds=SEEDS)
        walls = (ops_scenario.wall_grid(st.scenario.obstacles, wall[2], DEV), ops_scenario.wall_law(*wall[:2]))
        mlapm.MLAPM._run_scenario(st, sim._law(0.3), None, 8, walls=walls, nav=nav)
        runs.append(scenarios.scenario_result(st))
    assert all(_same(runs[0].member(m), runs[1].member(m)) and _same(runs[1].member(m), static_run().member(m)) for m in range(3))
    # ... and the stride is what separates the members: with it, members 1 and 2 read their own (infinite) planes
    dyn.member_stride = dyn.G * dyn.gy * dyn.gx
    st = scenarios.scenario_state_for(scene(), FRAMES, CAP, DEV, seeds=SEEDS)
    walls = (ops_scenario.wall_grid(st.scenario.obstacles, wall[2], DEV), ops_scenario.wall_law(*wall[:2]))
    mlapm.MLAPM._run_scenario(st, sim._law(0.3), None, 8, walls=walls, nav=dyn)
    own = scenarios.scenario_result(st)
    straight = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP)
    assert _same(own.member(0), static_run().member(0)) and _same(own.member(1), straight.member(1))
    st2 = scenarios.scenario_state_for(scene(), 4, CAP, DEV, seeds=SEEDS[:2])
    ops_scenario.scenario_step_mlapm(st2, None, init=True)
    with pytest.raises(ValueError, match='members'):
        ops_scenario.scenario_step_mlapm(st2, sim._law(0.3), nav=dyn)
    with pytest.raises(NotImplementedError):
        ops_scenario.scenario_step(st, torch.zeros_like(st.p), nav=dyn)          # the network-driven frame: not built


# ---- 6. behaviour: two rooms and two doors ----
# the wall on x = 5 is open over y in (1.25, 2.25), straight between the gates, and over y in (5.5, 7.0), a detour
DOOR_WALLS = [[[5.0, -2.0], [5.0, 1.25]], [[5.0, 2.25], [5.0, 5.5]], [[5.0, 7.0], [5.0, 9.5]]]
RATE, KD = 4.0, 2.0                                              # chosen from a first run (profiles/navdensity_summary.md)


def _crossings(res):
    """y of every recorded step across x = 5"""
    p, m = res.position.cpu().numpy().astype(np.float64), res.mask_p.cpu().numpy()
    a, b = p[:, :-1], p[:, 1:]
    both = (m[:, :-1] == 1) & (m[:, 1:] == 1)
    with np.errstate(invalid='ignore'):
        hit = both & ((a[..., 0] - 5.0) * (b[..., 0] - 5.0) < 0)
    w = (5.0 - a[..., 0][hit]) / (b[..., 0][hit] - a[..., 0][hit])
    return a[..., 1][hit] + w * (b[..., 1][hit] - a[..., 1][hit])


def test_a_queue_at_the_near_door_sends_agents_to_the_far_one():
    """pair forces off (A = 0): the outcome is the field's.  300 frames of dt = 0.08, cell 0.25, clearance 0.3, the default
    window (0.75 m, rho0 = 0.5 /m^2, fmax = 8, every 8 frames).  The wall term is on (Aw = 50, Bw = -5): an agent whose field
    turns under it can otherwise be carried into the blocked band beside the wall, where the lookup falls back to the straight
    line and walks it through the wall (in the first run without the term 18 of 157 crossings lay outside the doors).
    First run, 2 seeds: static 151 crossings, all near; kd = 2: 126 crossings, 64 of them (0.51) in the far door."""
    from piml_amd import ops_scenario, scenarios
    law = dict(WALLED, A=0.0, tau=0.5)
    sc = scenarios.floorplan_scenario(DOOR_WALLS, GATES, n_initial=10, rate_per_s=RATE).to(DEV)
    nav = ops_scenario.nav_field(sc, cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV)
    static = MLAPM(**law).simulate_ensemble(sc, 300, SEEDS[:2], capacity=256, nav=nav)
    dense = MLAPM(**law).simulate_ensemble(sc, 300, SEEDS[:2], capacity=256, nav=nav, nav_density=density(KD))
    assert static.dropped == [0, 0] and dense.dropped == [0, 0] and dense.spawned == static.spawned
    y0, y1 = _crossings(static), _crossings(dense)
    near = lambda y: (y > 1.25) & (y < 2.25)
    far = lambda y: (y > 5.5) & (y < 7.0)
    print(f'\n[navdensity] two doors, rate {RATE}/s: static {y0.size} crossings, {int(far(y0).sum())} far; kd = {KD}: {y1.size} '
          f'crossings, {int(far(y1).sum())} far ({far(y1).mean():.3f})')
    assert y0.size >= 100 and near(y0).all()                     # the static field: every crossing lies in the near door
    assert y1.size >= 100 and (near(y1) | far(y1)).all()         # none outside the two doors
    assert far(y1).any()                                         # ... and some in the far one
