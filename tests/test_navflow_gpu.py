"""GPU: the direction-aware density of the floor field (piml_nav_descent, piml_nav_flow, piml_nav_cost_flow,
piml_nav_relax_cost_gates; nav_density_law(flow=), MLAPM.simulate_*).  The deposit is the restatement's integers
(tests/navflow_ref.py), the descent direction, the cost planes and the solve its bits, before convergence as well; flow = 0 is
piml_nav_cost in every gate's plane and equal planes are piml_nav_relax_cost; the chain on the two-door plan sends the
prototype's probes to the prototype's doors, per gate; a run with flow = 0 is the run without the argument, and with flow = 1
members, captured replays and the sweep are bitwise each other."""
import functools

import numpy as np
import pytest
import torch

import nav_ref
import navcost_ref as COST
import navflow_ref as REF
from test_navdensity_gpu import BOUNDS, DEV, DOOR_WALLS, GATES, GRIDS, WALLED, MLAPM, dev, u32
from test_navflow import PROTO, PROTO_ROWS
from test_scenario_mlapm_gpu import _same, bits

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN, INF = float('nan'), float('inf')


def static_field(blocked, goal, x0=0.0, y0=0.0, cell=0.5):
    """the NavField of a hand-made grid, solved on the device (piml_nav_relax: nav_ref.solve's bits)"""
    from piml_amd import ops_scenario
    b, g = dev(blocked, goal)
    u, steps = ops_scenario.nav_relax(b, g)
    return ops_scenario.NavField(u, b, g, x0, y0, cell, 0.0, iterations=steps)


def grid_case(gx, gy, G):
    """blocked (gy, gx) and goal (G, gy, gx): the U shape with its two gates (and a third) on 33 x 34, scattered walls elsewhere"""
    rng = np.random.default_rng(gx * 100 + gy)
    if (gx, gy) == (33, 34):
        blocked, goal = nav_ref.u_shape_case()
        goal = np.concatenate([goal, np.zeros_like(goal[:1])])[:G]
        if G == 3:
            goal[2, 32, 16] = 1
        return blocked, np.ascontiguousarray(goal)
    blocked = (rng.uniform(size=(gy, gx)) < 0.15).astype(np.uint8)
    goal = np.zeros((G, gy, gx), np.uint8)
    for g, (y, x) in enumerate(((gy // 2, gx // 2), (0, 0), (gy - 1, gx - 1))[:G]):
        goal[g, y, x] = 1
    return blocked, goal


# ---- 1. the deposit ----

@pytest.mark.parametrize('members', [1, 3])
@pytest.mark.parametrize('cap', [1, 65, 300])
def test_deposit_is_the_restatement(cap, members):
    """7 x 5 cells of 0.25 from (-1, 2): positions on a cell boundary, on the outer edges, outside, NaN; velocities NaN, inf,
    +-20 m/s and halves of the unit; absent slots; dirty output planes"""
    from piml_amd import ops_scenario
    from test_navdensity_gpu import grid_field
    gx, gy, x0, y0, cell = 7, 5, -1.0, 2.0, 0.25
    rng = np.random.default_rng(100 * cap + members)
    P = np.stack([rng.uniform(x0 - 0.5, x0 + gx * cell + 0.5, (members, cap)),
                  rng.uniform(y0 - 0.5, y0 + gy * cell + 0.5, (members, cap))], -1).astype(f32)
    V = rng.normal(0, 1.5, (members, cap, 2)).astype(f32)
    inside = (x0 + 3 * cell, y0 + 2 * cell)                      # a cell boundary exactly: the cell (3, 2)
    special = [(inside, (0.5 / 1024, 1.5 / 1024)), (inside, (2.5 / 1024, -0.5 / 1024)), (inside, (NAN, 1.0)), (inside, (INF, -INF)),
               (inside, (20.0, -20.0)), (inside, (-20.0, 8.0)), ((x0, y0), (1.3, 0.0)), ((x0 + gx * cell, y0 + 0.1), (1.0, 1.0)),
               ((x0 + 0.1, y0 + gy * cell), (1.0, 1.0)), ((NAN, y0 + 0.1), (1.0, 1.0)), ((x0 + 0.1, NAN), (1.0, 1.0)),
               ((np.nextafter(f32(x0), f32(-9)), y0 + 0.1), (1.0, 1.0)), ((1e30, y0), (1.0, 1.0)), ((INF, y0 + 0.1), (1.0, 1.0)),
               ((x0 + 0.1, np.nextafter(f32(y0 + gy * cell), f32(0))), (-1.0, 3.0))]
    for m in range(members):
        for k, (p, v) in enumerate(special[m:]):                 # (capacity 1: member m gets special case m)
            if k < cap:
                P[m, k], V[m, k] = p, v
    mask = (rng.uniform(size=(members, cap)) < 0.8).astype(f32)
    mask[:, :min(cap, 8)] = 1
    field = grid_field(gx, gy, x0, y0, cell)
    want_c, want_m = REF.deposit_flow(P, V, mask, x0, y0, cell, gx, gy)
    pos, vel, msk = dev(P, V, mask)
    count, mom = ops_scenario.nav_flow(pos, vel, msk, field)
    assert count.dtype == mom.dtype == torch.int32 and tuple(mom.shape) == (members, 2, gy, gx)
    assert np.array_equal(count.cpu().numpy(), want_c) and np.array_equal(mom.cpu().numpy(), want_m)
    assert torch.equal(count, ops_scenario.nav_density(pos, msk, field))         # the count is nav_density's
    if cap > 1:
        assert 0 < want_c.sum() < mask.sum() and (want_m != 0).any()
    if cap > 8:
        assert want_m[0, 0, 2, 3] != 0 or want_m[0, 1, 2, 3] != 0
    dirty = torch.full_like(count, 7), torch.full_like(mom, -9)  # a second call on dirty planes: the entry zeroes all three
    out = ops_scenario.nav_flow(pos, vel, msk, field, out=dirty)
    assert out[0] is dirty[0] and out[1] is dirty[1] and torch.equal(dirty[0], count) and torch.equal(dirty[1], mom)
    if members == 1:                                             # a single run's state has no member axis
        one = ops_scenario.nav_flow(pos[0], vel[0], msk[0], field)
        assert torch.equal(one[0], count) and torch.equal(one[1], mom)


def test_deposit_of_300_agents_in_one_cell():
    from piml_amd import ops_scenario
    from test_navdensity_gpu import grid_field
    field = grid_field(7, 5, -1.0, 2.0, 0.25)
    P, V = np.empty((2, 300, 2), f32), np.empty((2, 300, 2), f32)
    P[0], V[0] = (-1.0 + 2.5 * 0.25, 2.0 + 3.5 * 0.25), (1.3, -0.7)
    P[1], V[1] = (-1.0 + 6.9 * 0.25, 2.0 + 0.1 * 0.25), (-20.0, 20.0)
    count, mom = ops_scenario.nav_flow(*dev(P, V), torch.ones(2, 300, device=DEV), field)
    want_c, want_m = np.zeros((2, 5, 7), np.int32), np.zeros((2, 2, 5, 7), np.int32)
    want_c[0, 3, 2], want_c[1, 0, 6] = 300, 300
    want_m[0, :, 3, 2] = 300 * 1331, 300 * -717
    want_m[1, :, 0, 6] = 300 * -8192, 300 * 8192
    assert np.array_equal(count.cpu().numpy(), want_c) and np.array_equal(mom.cpu().numpy(), want_m)
    assert np.array_equal(REF.deposit_flow(P, V, np.ones((2, 300), f32), -1.0, 2.0, 0.25, 7, 5)[1], want_m)


# ---- 2. the descent direction ----

@pytest.mark.parametrize('G', [1, 2, 3])
@pytest.mark.parametrize('gx,gy', GRIDS)
def test_descent_is_the_restatement(gx, gy, G):
    from piml_amd import ops_scenario
    blocked, goal = grid_case(gx, gy, G)
    field = static_field(blocked, goal)
    d = ops_scenario.nav_descent(field)
    assert tuple(d.shape) == (G, gy, gx, 2) and d.dtype == torch.float32
    u = field.u.cpu().numpy()
    want = REF.descent_dir(u)
    assert np.array_equal(u32(d), u32(want))
    assert (want[goal != 0] == 0).all() and (want[~np.isfinite(u)] == 0).all()
    if gx * gy > 40:
        assert (want != 0).any(axis=-1).sum() > gx * gy // 2
    dirty = torch.full_like(d, 3.0)
    assert ops_scenario.nav_descent(field, out=dirty) is dirty and torch.equal(bits(dirty), bits(d))


# ---- 3. the cost ----

def cost_inputs(gx, gy, seed, members=2, G=2):
    rng = np.random.default_rng(seed)
    count = rng.integers(0, 4, (members, gy, gx)).astype(np.int32)
    count[-1] = (rng.uniform(size=(gy, gx)) < 0.1) * rng.integers(1, 30, (gy, gx))
    mom = (rng.normal(0, 1300, (members, 2, gy, gx)) * count[:, None]).astype(np.int32)
    ang = rng.uniform(0, 2 * np.pi, (G, gy, gx))
    d = np.stack([np.cos(ang), np.sin(ang)], -1).astype(f32)
    d[rng.uniform(size=(G, gy, gx)) < 0.1] = 0                   # goal and blocked cells have no direction
    return count, mom, d


@pytest.mark.parametrize('r', [0, 1, 4, 8])
@pytest.mark.parametrize('gx,gy', GRIDS)
def test_cost_is_the_restatement(gx, gy, r):
    from piml_amd import ops_scenario
    from test_navdensity_gpu import grid_field
    cell = 0.5
    count, mom, d = cost_inputs(gx, gy, 1000 * gx + 10 * gy + r)
    field = grid_field(gx, gy, cell=cell, goal=np.zeros((2, gy, gx), np.uint8))
    c, m, dd = dev(count, mom, d)
    for flow, vref in ((1.0, 1.3), (0.5, 2.0)):
        law = ops_scenario.nav_density_law(2.0, rho0=0.5, radius=r * cell, fmax=8.0, flow=flow, vref=vref)
        want = REF.cost_flow(count, mom, d, cell, r, 2.0, 0.5, 8.0, flow, vref)
        got = ops_scenario.nav_cost_flow(c, m, dd, field, law)
        assert tuple(got.shape) == (2, 2, gy, gx) and np.array_equal(u32(got), u32(want)), (flow, vref)
        assert want.min() >= 1.0 and want.max() <= 8.0
    if gx * gy > 1:
        assert not np.array_equal(u32(want[:, 0]), u32(want[:, 1]))              # the gates do differ
    # flow = 0: every gate's plane is the scalar cost's, the restatement's and the device's
    law0 = ops_scenario.nav_density_law(2.0, rho0=0.5, radius=r * cell, fmax=8.0, flow=0.0)
    got0 = ops_scenario.nav_cost_flow(c, m, dd, field, law0, out=torch.full((2, 2, gy, gx), -1.0, device=DEV))
    scalar = ops_scenario.nav_cost(c, field, law0)
    want0, _ = COST.cost(count, cell, r, 2.0, 0.5, 8.0)
    for g in range(2):
        assert torch.equal(bits(got0[:, g]), bits(scalar)) and np.array_equal(u32(got0[:, g]), u32(want0)), g


def test_cost_at_rho0_at_fmax_and_below_zero():
    from piml_amd import ops_scenario
    from test_navdensity_gpu import grid_field
    count = np.zeros((1, 4, 5), np.int32)
    mom = np.zeros((1, 2, 4, 5), np.int32)
    count[0, 1, 1], count[0, 3, 4] = 9, 200
    mom[0, 0, 1, 1] = 9 * 2048                                   # nine walking +x at 2 m/s
    d = np.zeros((3, 4, 5, 2), f32)
    d[0, ..., 0], d[1, ..., 0], d[2, ..., 1] = 1.0, -1.0, 1.0    # gate 0 lies towards +x, gate 1 towards -x, gate 2 across
    field = grid_field(5, 4, cell=1.0, goal=np.zeros((3, 4, 5), np.uint8))
    c, m, dd = dev(count, mom, d)
    # vref = 1: s_eff = 9 - 18 < 0 for gate 0 (co-flow faster than vref), 9 + 18 for gate 1, 9 for gate 2: rho == rho0 exactly
    law = ops_scenario.nav_density_law(2.0, rho0=1.0, radius=1.0, fmax=8.0, flow=1.0, vref=1.0)
    want = REF.cost_flow(count, mom, d, 1.0, 1, 2.0, 1.0, 8.0, 1.0, 1.0)
    got = ops_scenario.nav_cost_flow(c, m, dd, field, law)
    assert np.array_equal(u32(got), u32(want))
    assert want[0, 0, 1, 1] == 1.0 and want[0, 1, 1, 1] == 5.0 and want[0, 2, 1, 1] == 1.0          # 1 + 2 (27 / 9 - 1)
    assert (want[0, :, 3, 4] == 8.0).all()                       # 200 standing in a cell: fmax for every gate
    sharp = ops_scenario.nav_cost_flow(c, m, dd, field, ops_scenario.nav_density_law(2.0, rho0=9.0, radius=0.0, fmax=1.0, flow=4.0))
    assert (sharp == 1.0).all()                                  # fmax = 1 clips everything


# ---- 4. the solve ----

@functools.lru_cache(maxsize=None)
def solve_case():
    """the U shape: blocked, goal (2 gates), cost (3 members, 2 gates, gy, gx), all six planes different, and the
    restatement's fixed points with their step counts, computed once"""
    blocked, goal = nav_ref.u_shape_case()
    rng = np.random.default_rng(77)
    cost = rng.uniform(1, 4, (3, 2) + blocked.shape).astype(f32)
    cost[2, 1] = 1.0 + 7.0 * (rng.uniform(size=blocked.shape) < 0.2)
    solved = [REF.solve_gates(blocked, goal, cost[m]) for m in range(3)]
    return blocked, goal, cost, np.stack([u for u, _ in solved]), [n for _, steps in solved for n in steps]


def test_solve_is_the_restatement_per_gate():
    """a cost indexed by member instead of by (member, gate), or by gate alone, would show"""
    from piml_amd import ops_scenario
    blocked, goal, cost, want, n = solve_case()
    b, g, c = dev(blocked, goal, cost)
    u, steps = ops_scenario.nav_relax_cost_gates(b, g, c)
    assert tuple(u.shape) == (3, 2, 34, 33) and steps % 128 == 0 and steps >= max(n)
    assert np.array_equal(u32(u), u32(want))
    assert len({u32(want[m, k]).tobytes() for m in range(3) for k in range(2)}) == 6
    one, _ = ops_scenario.nav_relax_cost_gates(b, g, c[1:2])
    assert np.array_equal(u32(one[0]), u32(want[1]))


@pytest.mark.parametrize('launches', [1, 3])
def test_solve_before_convergence_is_exact(launches):
    from piml_amd import ops_scenario
    blocked, goal, cost, _, n = solve_case()
    cases = [(blocked, goal, cost)]
    b65, g65 = grid_case(65, 65, 2)                              # three tiles a side
    cases.append((b65, g65, np.random.default_rng(65).uniform(1, 4, (3, 2, 65, 65)).astype(f32)))
    assert min(n) > 8 * launches                                 # not yet converged
    for blocked, goal, cost in cases:
        u, steps = ops_scenario.nav_relax_cost_gates(*dev(blocked, goal, cost), launches=launches)
        assert steps == 8 * launches
        for m in range(3):
            for k in range(2):
                want = COST.steps(nav_ref.start(goal[k:k + 1]), blocked, goal[k:k + 1], cost[m, k], 8 * launches)
                assert np.array_equal(u32(u[m, k]), u32(want[0])), (blocked.shape, m, k)


def test_equal_planes_are_nav_relax_cost_bit_for_bit():
    from piml_amd import ops_scenario
    for blocked, goal, cost in ((solve_case()[:3]), (*grid_case(65, 65, 2), np.random.default_rng(3).uniform(1, 4, (3, 2, 65, 65)).astype(f32))):
        b, g, c = dev(blocked, goal, cost)
        member = c[:, 0].contiguous()
        both = member.unsqueeze(1).repeat(1, 2, 1, 1).contiguous()
        for launches in (1, 3, None):
            want, n0 = ops_scenario.nav_relax_cost(b, g, member, launches=launches)
            got, n1 = ops_scenario.nav_relax_cost_gates(b, g, both, launches=launches)
            assert n0 == n1 and torch.equal(bits(got), bits(want)), (blocked.shape, launches)


def test_a_captured_batch_is_the_eager_one():
    from piml_amd import _lib, hip_graphs_safe
    assert hip_graphs_safe()
    blocked, goal, cost, want, n = solve_case()
    b, g, c = dev(blocked, goal, cost)
    start = torch.from_numpy(nav_ref.start(goal)).to(DEV).unsqueeze(0).repeat(3, 1, 1, 1).contiguous()
    ua, ub = start.clone(), torch.empty_like(start)
    changed = torch.zeros(6, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _lib.check(_lib.lib().piml_nav_relax_cost_gates(b.data_ptr(), g.data_ptr(), c.data_ptr(), ua.data_ptr(), ub.data_ptr(),
                                                            3, 2, 33, 34, 16, changed.data_ptr(), stream.cuda_stream),
                       'piml_nav_relax_cost_gates')
        graph.replay()
    torch.cuda.synchronize()
    assert max(n) <= 128 and np.array_equal(u32(ua), u32(want)) and changed.tolist() == [1] * 6
    changed.zero_()
    with torch.cuda.stream(stream):
        graph.replay()                                           # from the fixed point: nothing changes
    torch.cuda.synchronize()
    assert np.array_equal(u32(ua), u32(want)) and changed.tolist() == [0] * 6


# ---- 5. the chain on the device: two rooms, two doors, two gates ----

def test_chain_sends_the_probes_to_the_prototypes_doors():
    """positions and velocities placed by hand -> nav_field_update (deposit, cost per gate, solve per gate), each the
    restatement's bits -> nav_direction over the member's planes: every probe of every gate walks down its field in steps of
    half a cell until it stands on the wall's column.  The four rows of the prototype's table."""
    from piml_amd import ops_scenario
    blocked, goal, count = REF.two_door_two_gates()
    base = static_field(blocked, goal, cell=COST.TWO_DOOR_CELL)
    dyn = ops_scenario.NavFieldDynamic(base, 2, flow=True)
    d = REF.descent_dir(base.u.cpu().numpy())
    assert np.array_equal(u32(dyn.descent), u32(d))
    for (flow, vel), want_near in PROTO_ROWS:
        P, V = np.full((2, 32, 2), NAN, f32), np.full((2, 32, 2), NAN, f32)
        P[:, :25], V[:, :25] = COST.two_door_positions(), vel
        mask = np.zeros((2, 32), f32)
        mask[:, :25] = 1
        P[1, 30], V[1, 30], mask[1, 30] = (3.3, 3.3), (5.0, 5.0), 0              # an absent slot: not counted
        st = type('State', (), dict(zip(('p', 'v', 'mask'), dev(P, V, mask)), seeds=torch.zeros(2, dtype=torch.long, device=DEV)))()
        law = ops_scenario.nav_density_law(PROTO['kd'], rho0=PROTO['rho0'], radius=0.5, fmax=PROTO['fmax'], flow=flow, vref=PROTO['vref'])
        dyn.cost_gates.fill_(-1.0)
        steps = ops_scenario.nav_field_update(dyn, st, law)
        cnt, mom = REF.deposit_flow(P[:1], V[:1], mask[:1], 0.0, 0.0, COST.TWO_DOOR_CELL, 40, 24)
        f = REF.cost_flow(cnt, mom, d, COST.TWO_DOOR_CELL, PROTO['r'], PROTO['kd'], PROTO['rho0'], PROTO['fmax'], flow, PROTO['vref'])[0]
        if flow == 0.0:                                          # the scalar path: cost, not cost_gates, is written and read
            assert (dyn.cost_gates == -1.0).all()
            planes = dyn.cost.unsqueeze(1).expand(2, 2, 24, 40)
        else:
            planes = dyn.cost_gates
            assert np.array_equal(dyn.mom[0].cpu().numpy(), mom[0]) and torch.equal(dyn.mom[0], dyn.mom[1])
        u, n = REF.solve_gates(blocked, goal, f)
        assert steps == 256 and max(n) <= 128
        for m in range(2):
            assert np.array_equal(dyn.count[m].cpu().numpy(), count)
            assert np.array_equal(u32(planes[m]), u32(f)) and np.array_equal(u32(dyn.u[m]), u32(u)), (flow, vel, m)
        plane = dyn.member(1)
        for k, probes in enumerate((COST.TWO_DOOR_PROBES, REF.GATE1_PROBES)):
            p = torch.tensor([[(x + 0.5) * 0.5, (y + 0.5) * 0.5] for x, y in probes], device=DEV)
            gate = torch.full((7,), k, dtype=torch.int32, device=DEV)
            dest = torch.tensor([[18.25, 2.75], [1.75, 2.75]][k], device=DEV).repeat(7, 1)
            rows = torch.full((7,), -1, dtype=torch.long, device=DEV)
            for _ in range(200):
                p = p + 0.25 * ops_scenario.nav_direction(p, gate, dest, plane)
                col = torch.floor(p[:, 0] / 0.5)
                on_wall = ((col >= COST.TWO_DOOR_WALL) if k == 0 else (col <= COST.TWO_DOOR_WALL)) & (rows < 0)
                rows = torch.where(on_wall, torch.floor(p[:, 1] / 0.5).long(), rows)
            rows = rows.tolist()
            assert all(r in COST.NEAR_DOOR + COST.FAR_DOOR for r in rows), (flow, vel, k, rows)
            assert [r in COST.NEAR_DOOR for r in rows] == want_near[k], (flow, vel, k, rows)
    with pytest.raises(ValueError, match='flow=True'):           # a field built without the planes cannot take the law
        ops_scenario.nav_field_update(ops_scenario.NavFieldDynamic(base, 2), st, ops_scenario.nav_density_law(2.0, radius=0.5, flow=1.0))


# ---- 6. runs: the two-room, two-door floor plan ----
CAP, FRAMES, SEEDS = 128, 64, [0, 1]
LAWS = dict(WALLED, A=0.0, tau=0.5)


@functools.lru_cache(maxsize=None)
def scene():
    from piml_amd import scenarios
    return scenarios.floorplan_scenario(DOOR_WALLS, GATES, n_initial=10, rate_per_s=4.0).to(DEV)


@functools.lru_cache(maxsize=None)
def field():
    from piml_amd import ops_scenario
    return ops_scenario.nav_field(scene(), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV)


def density(**kw):
    from piml_amd import ops_scenario
    return ops_scenario.nav_density_law(2.0, rho0=0.0, **kw)      # rho0 = 0: every agent raises the cost around it


@functools.lru_cache(maxsize=None)
def flow_run():
    return MLAPM(**LAWS).simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(flow=1.0))


def test_flow_zero_is_the_run_without_the_argument():
    sim = MLAPM(**LAWS)
    plain = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density())
    zero = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=density(flow=0.0, vref=2.0))
    assert all(_same(zero.member(m), plain.member(m)) for m in range(2))
    assert not any(_same(flow_run().member(m), plain.member(m)) for m in range(2))      # ... and flow = 1 is another run
    assert flow_run().spawned == plain.spawned and flow_run().dropped == [0, 0]


def test_members_captured_replays_and_the_sweep_are_each_other():
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    sim, law = MLAPM(**LAWS), density(flow=1.0)
    ens = flow_run()
    for m, s in enumerate(SEEDS):
        one = sim.simulate_scenario(scene(), FRAMES, seed=s, capacity=CAP, nav=field(), nav_density=law)
        assert _same(ens.member(m), one), m                      # member m is the single run of its seed
    graph = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=law, use_graph=True)
    eager = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), nav_density=law, use_graph=False)
    table = sim.simulate_sweep(scene(), FRAMES, [LAWS], SEEDS, capacity=CAP, nav=field(), nav_density=law)
    for m in range(2):
        assert _same(graph.member(m), eager.member(m)) and _same(graph.member(m), ens.member(m)), m
        assert _same(table.member(m), ens.member(m)), m


def test_the_exit_choice_in_front_of_it_runs_captured_as_eager():
    from piml_amd import ops_scenario
    sim, law = MLAPM(**LAWS), density(flow=1.0)
    choice = ops_scenario.exit_choice_law([[0, 1]], margin=0.0, commit=0.0, every=8)
    kw = dict(capacity=CAP, nav=field(), nav_density=law, exit_choice=choice)
    graph = sim.simulate_ensemble(scene(), FRAMES, SEEDS, use_graph=True, **kw)
    eager = sim.simulate_ensemble(scene(), FRAMES, SEEDS, use_graph=False, **kw)
    assert all(_same(graph.member(m), eager.member(m)) for m in range(2))
    assert graph.spawned == flow_run().spawned
