"""GPU: the floor-field solve by active tiles (piml_nav_relax_active; nav_density_law(solver='active'), MLAPM.simulate_*).  On
one-cell, one-row, edge-tile and nine-tile grids and on the re-activation case, with three members of different costs, two
gates and both cost forms: the field is the dense entries' fixed point bit for bit, the work per plane the restatement's
integers (tests/navactive_ref.py), both buffers are equal and stalled is 0; after 2 and 4 launches the field is the dense
kernels' after the same launches; too few launches set stalled and it stays set; a captured call is the eager one, on dirty
flags and work too; a run under solver='active' is the run under solver='batch', captured or not, and a captured run takes
an update interval that divides the frames of its graph."""
import functools

import numpy as np
import pytest
import torch

import navactive_ref as REF
from test_navdensity_gpu import BOUNDS, DEV, DOOR_WALLS, GATES, SEEDS, WALLED, MLAPM, u32
from test_scenario_mlapm_gpu import _same

pytestmark = pytest.mark.gpu
FRAMES, CAP = 60, 128


def dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)         # (a copy: the cases are read-only)


def even(n):
    return max(2, n + (n & 1))


def buffers(goal, members, dirty=False):
    """(u_a with the cold start, u_b, flags, work, stalled) for `members` members of goal (G, gy, gx) on the device"""
    from piml_amd import ops_scenario
    G, gy, gx = (int(n) for n in goal.shape)
    a = torch.where(goal != 0, 0.0, float('inf')).to(torch.float32).unsqueeze(0).repeat(members, 1, 1, 1).contiguous()
    b = torch.full_like(a, float('nan'))
    flags, work, stalled = ops_scenario.nav_active_buffers(members * G, gy, gx, DEV)
    if dirty:
        flags.fill_(1)
        flags[1].fill_(-7)
    return a, b, flags, work, stalled


# ---- 1. the fixed point, the work and the buffers ----

@pytest.mark.parametrize('name', REF.CASES)
@pytest.mark.parametrize('gates', (False, True))
def test_field_is_the_dense_fixed_point_and_work_the_restatement(name, gates):
    from piml_amd import ops_scenario
    blocked, goal, c3, c4 = REF.case(name)
    ref = REF.solved(name, gates)
    b, g, c = dev(blocked, goal, c4 if gates else c3)
    want, _ = (ops_scenario.nav_relax_cost_gates if gates else ops_scenario.nav_relax_cost)(b, g, c)
    n = even(ref.launches)
    ua, ub, flags, work, stalled = buffers(g, 3, dirty=True)
    ops_scenario._relax_active(b, g, c, ua, ub, flags, work, stalled, n)
    assert np.array_equal(u32(ua), u32(want)) and np.array_equal(u32(ua), u32(ref.u))
    assert np.array_equal(u32(ua), u32(ub))                  # the fixed point is in both buffers
    assert np.array_equal(work.cpu().numpy().reshape(3, 2), ref.work)
    assert int(stalled.item()) == 0
    assert ((flags == 0) | (flags == 1)).all().item()        # every word of the dirty planes was written again
    assert not flags[(n - 1) & 1].any().item()               # the last launch changed nothing
    # the operator: its own buffers, more launches than needed -- they step nothing
    u, wk, st = ops_scenario.nav_relax_active(b, g, c, n + 6)
    assert np.array_equal(u32(u), u32(want)) and np.array_equal(wk.cpu().numpy(), ref.work) and int(st.item()) == 0
    assert tuple(u.shape) == (3, 2) + blocked.shape and tuple(wk.shape) == (3, 2) and wk.dtype == torch.int32


@pytest.mark.parametrize('name', ('33x34', '65x65', 'reactivation'))
@pytest.mark.parametrize('gates', (False, True))
def test_partial_runs_are_the_dense_kernels(name, gates):
    from piml_amd import ops_scenario
    blocked, goal, c3, c4 = REF.case(name)
    b, g, c = dev(blocked, goal, c4 if gates else c3)
    dense = ops_scenario.nav_relax_cost_gates if gates else ops_scenario.nav_relax_cost
    for n in (2, 4):
        want, steps = dense(b, g, c, launches=n)
        got, work, stalled = ops_scenario.nav_relax_active(b, g, c, n)
        assert steps == 8 * n and np.array_equal(u32(got), u32(want)), n
        ref = REF.relax_active(blocked, goal, c4 if gates else c3, launches=n)
        assert np.array_equal(u32(got), u32(ref.u)) and np.array_equal(work.cpu().numpy(), ref.work)
        assert bool(stalled.item()) == ref.stalled


# ---- 2. stalled ----

def test_too_few_launches_set_stalled_and_it_stays_set():
    from piml_amd import ops_scenario
    blocked, goal, c3, _ = REF.case('reactivation')
    ref = REF.solved('reactivation', False)
    b, g, c = dev(blocked, goal, c3)
    ua, ub, flags, work, stalled = buffers(g, 3)
    ops_scenario._relax_active(b, g, c, ua, ub, flags, work, stalled, 2)
    assert int(stalled.item()) == 1
    ua.copy_(buffers(g, 3)[0])                               # a further call, from the cold start, that converges
    work.zero_()
    ops_scenario._relax_active(b, g, c, ua, ub, flags, work, stalled, even(ref.launches))
    assert np.array_equal(u32(ua), u32(ref.u)) and np.array_equal(work.cpu().numpy().reshape(3, 2), ref.work)
    assert int(stalled.item()) == 1                          # the entry never clears it
    assert ops_scenario.nav_relax_active(b, g, c, even(ref.launches))[2].item() == 0


def test_the_entry_takes_the_values_the_refusals_start_from():
    """tests/test_navactive.py refuses each of these values changed in one thing; unchanged they run"""
    from piml_amd import _lib
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    blocked, goal = torch.zeros(4, dtype=torch.uint8, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV)
    cost, a, b = torch.ones(4, device=DEV), torch.full((4,), float('inf'), device=DEV), torch.zeros(4, device=DEV)
    with torch.cuda.device(DEV):
        s = torch.cuda.current_stream().cuda_stream
        for work in (z[40:].data_ptr(), None):
            assert _lib.lib().piml_nav_relax_active(blocked.data_ptr(), goal.data_ptr(), cost.data_ptr(), 0, a.data_ptr(), b.data_ptr(),
                                                    1, 1, 2, 2, 2, z.data_ptr(), work, z[32:].data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert z[40].item() == 1 and z[32].item() == 0 and torch.isinf(a).all().item()     # no goal: one tile stepped once, nothing moved


# ---- 3. capture ----

def test_a_captured_call_is_the_eager_call():
    from piml_amd import hip_graphs_safe, ops_scenario
    assert hip_graphs_safe()
    blocked, goal, _, c4 = REF.case('reactivation')
    ref = REF.solved('reactivation', True)
    b, g, c = dev(blocked, goal, c4)
    n = even(ref.launches)
    ua, ub, flags, work, stalled = buffers(g, 3)
    start = ua.clone()
    ops_scenario._relax_active(b, g, c, ua, ub, flags, work, stalled, n)        # eager; leaves flags and work dirty
    eager, eager_work = ua.clone(), work.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # no host read, no allocation: the call is capturable as it is
        ua.copy_(start)
        ops_scenario._relax_active(b, g, c, ua, ub, flags, work, stalled, n)
    for k in range(2):
        ub.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(ua), u32(eager)) and np.array_equal(u32(ua), u32(ref.u)) and np.array_equal(u32(ub), u32(ua))
        assert torch.equal(work, eager_work * (k + 2))       # work is only added to: the caller clears it
        assert int(stalled.item()) == 0


# ---- 4. runs: the two-door plan ----

@functools.lru_cache(maxsize=None)
def scene():
    from piml_amd import scenarios
    return scenarios.floorplan_scenario(DOOR_WALLS, GATES, n_initial=10, rate_per_s=4.0).to(DEV)


@functools.lru_cache(maxsize=None)
def field():
    from piml_amd import ops_scenario
    return ops_scenario.nav_field(scene(), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV)


def density(solver, **kw):
    """rho0 = 0: every agent raises the cost around it, so the fields differ from the static one from the first update"""
    from piml_amd import ops_scenario
    return ops_scenario.nav_density_law(4.0, rho0=0.0, solver=solver, **kw)


def run(solver, use_graph, **kw):
    return MLAPM(**WALLED).simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), use_graph=use_graph,
                                             nav_density=density(solver, **kw))


@functools.lru_cache(maxsize=None)
def batch_run(every=8, flow=0.0):
    return run('batch', False, every=every, flow=flow)


def same_run(a, b):
    return all(_same(a.member(m), b.member(m)) for m in range(len(SEEDS)))


def test_the_active_run_is_the_batch_run():
    sim = MLAPM(**WALLED)
    static = sim.simulate_ensemble(scene(), FRAMES, SEEDS, capacity=CAP, nav=field(), use_graph=False)
    assert not same_run(batch_run(), static)                 # the term acts on this plan
    ens = run('active', False)
    assert same_run(ens, batch_run())
    law = density('active')
    one = sim.simulate_scenario(scene(), FRAMES, seed=SEEDS[1], capacity=CAP, nav=field(), nav_density=law, use_graph=False)
    assert _same(one, batch_run().member(1))
    table = sim.simulate_sweep(scene(), FRAMES, [WALLED], SEEDS, capacity=CAP, nav=field(), nav_density=law, use_graph=False)
    assert same_run(table, batch_run())
    assert same_run(run('active', False, flow=1.0), batch_run(flow=1.0))        # the cost plane per gate
    assert not same_run(batch_run(flow=1.0), batch_run())


def test_captured_between_replays_is_the_eager_run():
    assert same_run(run('active', True), batch_run()) and same_run(run('active', True, every=16), batch_run(every=16))


@pytest.mark.parametrize('every', (2, 4))
def test_an_update_captured_with_its_frames_is_the_eager_run(every):
    """every divides frames_per_graph = 8: ValueError before solver='active'"""
    graph = run('active', True, every=every)
    assert same_run(graph, run('active', False, every=every)) and same_run(graph, batch_run(every=every))
    assert not same_run(graph, batch_run())                  # (another schedule is another run)
    if every == 2:
        table = MLAPM(**WALLED).simulate_sweep(scene(), FRAMES, [WALLED], SEEDS, capacity=CAP, nav=field(), use_graph=True,
                                               nav_density=density('active', every=2, flow=1.0))
        assert same_run(table, batch_run(every=2, flow=1.0))


def test_other_intervals_are_still_refused():
    for solver in ('batch', 'active'):
        with pytest.raises(ValueError, match='multiple of frames_per_graph'):
            run(solver, True, every=3)
    with pytest.raises(ValueError, match='multiple of frames_per_graph'):
        run('batch', True, every=2)
    assert same_run(run('active', False, every=3), batch_run(every=3))          # (an eager run takes any interval)


def test_check_converged_raises_when_the_launches_were_too_few():
    from piml_amd import ops_scenario, scenarios
    with pytest.raises(RuntimeError, match='max_launches = 2'):
        run('active', False, max_launches=2)                 # 16 steps do not cross a 52-cell grid
    dyn = ops_scenario.NavFieldDynamic(field(), len(SEEDS))
    st = scenarios.scenario_state_for(scene(), 4, CAP, DEV, seeds=SEEDS)
    ops_scenario.scenario_step_mlapm(st, None, init=True)
    assert ops_scenario.nav_field_update(dyn, st, density('active', max_launches=2)) == 16 and dyn.max_launches == 2
    with pytest.raises(RuntimeError, match='max_launches'):
        dyn.check_converged()
    steps = ops_scenario.nav_field_update(dyn, st, density('active'))           # the default bound converges here ...
    assert steps == 8 * dyn.default_max_launches() == dyn.iterations and dyn.updates == 2
    assert np.array_equal(u32(dyn.u), u32(dyn.u_b))
    with pytest.raises(RuntimeError):                        # ... and the word stays set until the run's reset
        dyn.check_converged()
    want = dyn.u.clone()
    dyn.reset()
    dyn.check_converged()
    ops_scenario.nav_field_update(dyn, st, density('batch'))
    assert np.array_equal(u32(dyn.u), u32(want))
    tiles = dyn.flags.shape[2] * dyn.flags.shape[3]
    ops_scenario.nav_field_update(dyn, st, density('active'))
    work = dyn.work.cpu().numpy()
    assert np.array_equal(u32(dyn.u), u32(want)) and (work >= tiles).all() and (work < dyn.max_launches * tiles).all()
    dyn.check_converged()
