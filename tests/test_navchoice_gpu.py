"""GPU: the exit choice (piml_nav_choose_exit; ops_scenario.nav_choose_exit; MLAPM.simulate_*(..., exit_choice=);
ops_scenario.scenario_step(nav=) with the choice in front).  The kernel against the numpy restatement (tests/navchoice_ref.py)
bit for bit on states that hold every case of the rule (tests/navchoice_cases.py), at every size at which the launch takes
another shape; frames with the choice in front against the same frames on a state the restatement rewrote; runs against
runs; and two behaviours: routed agents leave by the nearer of two equivalent exits, and by the far one when the near one is
queued and the field carries the density term."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import navchoice_cases as CASES
import navchoice_ref as REF
import navcost_ref
from conftest import REPO
from test_scenario_mlapm_gpu import LAW, _same, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32
STATE = ('p', 'v', 'a', 'dest', 'flag', 'mask', 'waypoints', 'exit_idx', 'desired_speed', 'hist', 'selff', 'spawned', 'spawn_count',
         'dropped', 'p_res', 'v_res', 'a_res', 'dest_res', 'mask_res', 'spawn_iters')
WRITTEN = ('dest', 'waypoints', 'exit_idx')                      # what the choice may write


def _scenario(entries, **kw):
    from piml_amd import scenarios
    fields = dict(route_max_iters=0, num_waypoints=CASES.D_ROWS, spawn_offset=CASES.SPAWN_OFFSET, n_initial=0, name='navchoice')
    fields.update(kw)
    return scenarios.Scenario(entries=torch.from_numpy(np.ascontiguousarray(entries)), route_polyline=torch.zeros(2, 2),
                              obstacles=torch.zeros(0, 2), **fields).to(DEV)


def _put(st, states, t):
    """the per-member numpy states into st, at frame counter t"""
    lead = st.members is not None
    stack = lambda k: torch.from_numpy(np.stack([s[k] for s in states]) if lead else states[0][k]).to(DEV)
    for name, k in (('p', 'p'), ('dest', 'dest'), ('flag', 'flag'), ('mask', 'mask'), ('waypoints', 'waypoints'),
                    ('exit_idx', 'exit_idx')):
        getattr(st, name).copy_(stack(k))
    st.t.fill_(t)
    st.spawned[..., t & 1] = states[0]['n']
    st.spawned[..., (t + 1) & 1] = 0                             # the other parity is not the frame's: nobody is live under it


def _state(case, t=CASES.T_ON):
    from piml_amd import ops_scenario
    members = len(case['states'])
    kw = dict(seed=case['seeds'][0]) if members == 1 else dict(seeds=case['seeds'])
    st = ops_scenario.scenario_state(_scenario(case['entries']), case['states'][0]['p'].shape[0], 4, **kw)
    _put(st, case['states'], t)
    return st


def _field(case, per_member=True):
    """a NavFieldDynamic over the case's per-member planes, or the static NavField of member 0's"""
    from piml_amd import ops_scenario
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    base = ops_scenario.NavField(dev(case['u'][0]), dev(case['blocked']), dev(case['goal']), CASES.X0, CASES.Y0, CASES.CELL, 2.0)
    if not per_member:
        return base
    dyn = ops_scenario.NavFieldDynamic(base, len(case['states']))
    dyn.u.copy_(dev(case['u']))
    return dyn


def _law(G, margin=CASES.MARGIN):
    from piml_amd import ops_scenario
    return ops_scenario.exit_choice_law(CASES.classes_of(G), margin=margin, commit=CASES.COMMIT, every=CASES.EVERY)


def _snapshot(st):
    return {k: getattr(st, k).clone() for k in STATE}


def _assert_state(st, before, want=None, what=''):
    """every tensor of st is bitwise `before`'s, but for WRITTEN, which are the restatement's `want` (a list of member states)"""
    torch.cuda.synchronize()
    lead = st.members is not None
    for k in STATE:
        got = getattr(st, k)
        if want is not None and k in WRITTEN:
            ref = torch.from_numpy(np.stack([s[k] for s in want]) if lead else want[0][k]).to(DEV)
        else:
            ref = before[k]
        assert torch.equal(bits(got), bits(ref)), (what, k, int((bits(got) != bits(ref)).sum()))


# ---- 1. the kernel is the restatement ----

@pytest.mark.parametrize('grid', list(CASES.GRIDS))
@pytest.mark.parametrize('G', [3, 64])
@pytest.mark.parametrize('members', [1, 3])
@pytest.mark.parametrize('cap', [1, 65, 300])
def test_kernel_is_the_restatement(cap, members, G, grid):
    """per-member fields of different cost; every case of the rule in one state; the switch counts on top of what was there"""
    from piml_amd import ops_scenario
    case = CASES.build(cap, members, G, grid)
    want, switched = CASES.expected(case)
    st, field, law = _state(case), _field(case), _law(G)
    before = _snapshot(st)
    count = torch.full_like(st.flag, 7)
    ops_scenario.nav_choose_exit(st, field, law, count)
    _assert_state(st, before, want, 'scheduled')
    sw = torch.from_numpy(switched if members > 1 else switched[0]).to(DEV)
    assert torch.equal(count, 7 + sw)
    if cap >= 65:
        assert 0 < int(switched.sum()) < switched.size
    # without a count: the same state
    again = _state(case)
    ops_scenario.nav_choose_exit(again, field, law)
    _assert_state(again, before, want, 'no count')
    # no gate in any class: nothing moves
    none = _state(case)
    desc = law.desc(field.cell)
    cls = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    from piml_amd import _lib
    _lib.check(_lib.lib().piml_nav_choose_exit(ctypes.byref(none.desc), none.seeds.numel(), none.seeds.data_ptr(),
                                               ctypes.byref(field.desc), field.member_stride, cls.data_ptr(), ctypes.byref(desc),
                                               None, 0, torch.cuda.current_stream().cuda_stream), 'piml_nav_choose_exit')
    _assert_state(none, before, None, 'all -1')


@pytest.mark.parametrize('t,offset', [(CASES.T_OFF, 0), (0, 0), (CASES.T_ON + 1, 0), (CASES.T_ON, 1), (2, 5)])
def test_unscheduled_frames_leave_the_state_untouched(t, offset):
    from piml_amd import ops_scenario
    case = CASES.build(65, 3, 3, 'ushape')
    st, field = _state(case, t), _field(case)
    before = _snapshot(st)
    count = torch.zeros_like(st.flag)
    ops_scenario.nav_choose_exit(st, field, _law(3), count, frame_offset=offset)
    _assert_state(st, before, None, (t, offset))
    assert int(count.sum()) == 0


def test_the_frame_offset_counts_towards_the_schedule():
    """counter 4 + offset 5 is frame 9: the pass a captured graph's sixth frame makes"""
    from piml_amd import ops_scenario
    case = CASES.build(65, 3, 3, 'ushape')
    want, switched = CASES.expected(case)
    st, field = _state(case, CASES.T_ON), _field(case)
    before = _snapshot(st)
    st.t.fill_(4)
    ops_scenario.nav_choose_exit(st, field, _law(3), frame_offset=5)
    _assert_state(st, before, want, 'offset')
    assert switched.sum() > 0


def test_stride_zero_reads_the_one_static_field():
    from piml_amd import ops_scenario
    case = CASES.build(65, 3, 64, 'big')
    want, switched = CASES.expected(case, shared_field=True)
    own, _ = CASES.expected(case)
    st = _state(case)
    before = _snapshot(st)
    ops_scenario.nav_choose_exit(st, _field(case, per_member=False), _law(64))
    _assert_state(st, before, want, 'static')
    assert any(not np.array_equal(a['exit_idx'], b['exit_idx']) for a, b in zip(want[1:], own[1:]))    # the members' own differ


def test_an_infinite_margin_still_leaves_an_unreachable_gate():
    from piml_amd import ops_scenario
    case = CASES.build(65, 3, 3, 'row')
    want, switched = CASES.expected(case, margin=f32(np.inf))
    st = _state(case)
    before = _snapshot(st)
    ops_scenario.nav_choose_exit(st, _field(case), _law(3, margin=float('inf')))
    _assert_state(st, before, want, 'inf')
    named = case['case'] == CASES.CASES.index('cur_unreachable')
    assert switched[named].sum() > 0
    for m, i in np.argwhere(switched == 1):                      # (a background slot may stand on such a cell too)
        s = case['states'][m]
        cx, cy = REF.cell_of(s['p'][i], CASES.X0, CASES.Y0, CASES.CELL, case['gx'], case['gy'])
        assert not np.isfinite(case['u'][m, s['exit_idx'][s['flag'][i], i], cy, cx]), (m, i)


def test_a_captured_launch_is_the_eager_one():
    import piml_amd
    from piml_amd import ops_scenario
    if not piml_amd.hip_graphs_safe():
        pytest.skip('HIP graph capture is not safe in this process')
    case = CASES.build(300, 3, 64, 'ushape')
    want, switched = CASES.expected(case)
    st, field, law = _state(case), _field(case), _law(64)
    before = _snapshot(st)
    count = torch.zeros_like(st.flag)
    idle = _state(case, CASES.T_OFF)
    ops_scenario.nav_choose_exit(idle, field, law, count)        # the library and the law's table are warm; nothing moved
    assert int(count.sum()) == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops_scenario.nav_choose_exit(st, field, law, count)
    _assert_state(st, before, None, 'captured, not run')
    graph.replay()
    _assert_state(st, before, want, 'replayed')
    assert torch.equal(count, torch.from_numpy(switched).to(DEV))
    graph.replay()                                               # a second pass on the result: whoever switched stays
    again, sw2 = [], []
    for m, s in enumerate(want):
        new, w = REF.choose(s, case['u'][m], CASES.X0, CASES.Y0, CASES.CELL, case['classes'], case['margin'], case['commit'],
                            CASES.EVERY, CASES.T_ON, case['seeds'][m], case['entries'], CASES.SPAWN_OFFSET)
        again.append(new)
        sw2.append(w)
    _assert_state(st, before, again, 'replayed twice')
    assert torch.equal(count, torch.from_numpy(switched + np.stack(sw2)).to(DEV))


def test_python_refusals_on_a_state():
    from piml_amd import ops_scenario
    case = CASES.build(65, 3, 3, 'row')
    st, field = _state(case), _field(case)
    with pytest.raises(TypeError):
        ops_scenario.nav_choose_exit(st, field, [[0, 2]])
    with pytest.raises(TypeError):
        ops_scenario.nav_choose_exit(st, None, _law(3))
    with pytest.raises(ValueError, match='outside'):
        ops_scenario.nav_choose_exit(st, field, ops_scenario.exit_choice_law([[0, 3]]))
    with pytest.raises(ValueError):
        ops_scenario.nav_choose_exit(st, field, _law(3), switch_count=torch.zeros(65, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops_scenario.nav_choose_exit(st, field, _law(3), switch_count=torch.zeros_like(st.mask))
    with pytest.raises(ValueError):
        ops_scenario.nav_choose_exit(st, field, _law(3), frame_offset=-1)
    one = _state(CASES.build(65, 1, 3, 'row'))
    with pytest.raises(ValueError, match='members'):
        ops_scenario.nav_choose_exit(one, field, _law(3))


# ---- 2. frames with the choice in front ----

HALL_WALLS = [[[0.0, 0.0], [20.0, 0.0], [20.0, 10.0], [0.0, 10.0], [0.0, 0.0]]]
HALL_GATES = [[[0.6, 4.0], [0.6, 6.0]], [[4.0, 0.6], [6.0, 0.6]], [[19.4, 4.0], [19.4, 6.0]]]    # A, the near exit, the far exit
HALL_BOUNDS = (-0.5, -0.5, 20.5, 10.5)
HALL_CELL = 0.5


@functools.lru_cache(maxsize=None)
def hall(n_initial=10, rate=2.0):
    from piml_amd import scenarios
    return scenarios.floorplan_scenario(HALL_WALLS, HALL_GATES, n_initial=n_initial, rate_per_s=rate, arrival_radius=0.5,
                                        spawn_offset=0.4, exits=[[1, 2]]).to(DEV)


@functools.lru_cache(maxsize=None)
def hall_field():
    from piml_amd import ops_scenario
    return ops_scenario.nav_field(hall(), cell=HALL_CELL, clearance=0.3, bounds=HALL_BOUNDS, device=DEV)


def _restate(st, field, law, t):
    """the restatement on st's state as it stands: -> (member states, switched)"""
    u = field.u.cpu().numpy()
    if u.ndim == 3:
        u = np.broadcast_to(u, (st.seeds.numel(), *u.shape))
    lead = st.members is not None
    host = {k: getattr(st, n).cpu().numpy() for k, n in (('p', 'p'), ('dest', 'dest'), ('flag', 'flag'), ('mask', 'mask'),
                                                         ('waypoints', 'waypoints'), ('exit_idx', 'exit_idx'))}
    spawned = st.spawned.cpu().numpy().reshape(-1, 2)
    seeds = st.seed_list if lead else [st.seed]
    out, sw = [], []
    ent = st.scenario.entries.cpu().numpy()
    cls = REF.gate_class(law.classes, ent.shape[0])
    for m, seed in enumerate(seeds):
        s = {k: (v[m] if lead else v) for k, v in host.items()}
        s['n'] = int(spawned[m, t & 1])
        new, w = REF.choose(s, u[m], field.x0, field.y0, field.cell, cls, REF.cells(law.margin, field.cell),
                            REF.cells(law.commit, field.cell), law.every, t, seed, ent, float(st.scenario.spawn_offset))
        out.append(new)
        sw.append(w)
    return out, np.stack(sw)


def _rewrite(st, states):
    lead = st.members is not None
    for k in WRITTEN:
        getattr(st, k).copy_(torch.from_numpy(np.stack([s[k] for s in states]) if lead else states[0][k]).to(DEV))


@pytest.mark.parametrize('form', ['ensemble', 'single', 'table'])
def test_one_mlapm_frame_with_the_choice_in_front(form):
    """two states run to the scheduled counter value 9 alike; A takes the choice launch and the frame, B is rewritten by the
    restatement and takes the frame alone: every tensor and record is bitwise the same"""
    from piml_amd import ops_scenario, scenarios
    sc, nav = hall(), hall_field()
    choice = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)
    kw = dict(seed=3) if form == 'single' else dict(seeds=[3, 4, 5])
    mlaw = ops_scenario.mlapm_law('GC', **LAW)
    A, B = (scenarios.scenario_state_for(sc, 16, 48, DEV, **kw) for _ in range(2))
    if form == 'table':
        mlaw = ops_scenario.mlapm_law_table([ops_scenario.mlapm_law('GC', **dict(LAW, tau=0.4 + 0.1 * m)) for m in range(3)], DEV)
    for st in (A, B):
        ops_scenario.scenario_step_mlapm(st, None, init=True)
        for _ in range(9):
            ops_scenario.scenario_step_mlapm(st, mlaw, nav=nav)
    assert int(A.t.item()) == 9
    before = _snapshot(B)
    want, switched = _restate(B, nav, choice, 9)
    assert switched.sum() >= 2                                   # agents bound for the far exit that stand nearer the near one
    ops_scenario.nav_choose_exit(A, nav, choice, ops_scenario.scenario_exit_switches(A))
    _assert_state(A, before, want, 'choice')
    assert torch.equal(A.exit_switches, torch.from_numpy(switched if form != 'single' else switched[0]).to(DEV))
    _rewrite(B, want)
    for st in (A, B):
        ops_scenario.scenario_step_mlapm(st, mlaw, nav=nav)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(bits(getattr(A, k)), bits(getattr(B, k))), k
    assert int(A.t.item()) == 10


@pytest.mark.parametrize('where', ['plan', 'hall'])
def test_one_network_driven_routed_frame_with_the_choice_in_front(where):
    """ops_scenario.scenario_step(nav=) as BaseSimulator._run_scenario calls it, the choice launch in front: the frame computes
    st.steer from exit_idx after the move, so the target follows the new gate in the same frame.  The accelerations are random
    numbers in the network's place (the frame reads them as data), the oracle approach of test_scenario_routed_gpu.py's twins.
    'plan' is that file's own scene and field: two gates, so the one candidate of an agent is the gate it is bound for and the
    pass must leave the state alone; 'hall' has two exits in a class and agents that switch"""
    from piml_amd import ops_scenario, scenarios
    if where == 'plan':
        from test_scenario_nav_gpu import CAP, SEEDS, field, scene
        sc, nav, cap, seeds = scene('plan'), field('plan'), CAP, SEEDS
        choice = ops_scenario.exit_choice_law([[0, 1]], margin=0.0, commit=0.0, every=8)
    else:
        sc, nav, cap, seeds = hall(), hall_field(), 48, [3, 4, 5]
        choice = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)
    A, B = (scenarios.scenario_state_for(sc, 16, cap, DEV, seeds=seeds) for _ in range(2))
    gen = torch.Generator(device=DEV).manual_seed(0)
    acc = [torch.randn(3, cap, 2, device=DEV, generator=gen) for _ in range(10)]
    for st in (A, B):
        ops_scenario.scenario_step(st, init=True, nav=nav)
        for k in range(9):
            ops_scenario.scenario_step(st, acc[k], nav=nav)
            st.t.add_(1)
    before = _snapshot(B)
    want, switched = _restate(B, nav, choice, 9)
    assert switched.sum() >= 2 if where == 'hall' else switched.sum() == 0
    ops_scenario.nav_choose_exit(A, nav, choice)
    _assert_state(A, before, want, 'choice')
    _rewrite(B, want)
    for st in (A, B):
        ops_scenario.scenario_step(st, acc[9], nav=nav)
    torch.cuda.synchronize()
    for k in STATE + ('steer',):
        assert torch.equal(bits(getattr(A, k)), bits(getattr(B, k))), k
    # and the target did follow: a switched, still present slot steers by the new gate's plane
    if where == 'plan':
        return
    still = torch.from_numpy(switched == 1).to(DEV) & (A.mask == 1)
    assert int(still.sum()) >= 1
    now = torch.gather(A.exit_idx, 1, A.flag.clamp(max=1).long().unsqueeze(1)).squeeze(1)
    assert (now[still] == 1).all() and not A.steer[still].isnan().any()


# ---- 3. runs ----

def _mlapm(**kw):
    from piml_amd.models.mlapm import MLAPM
    return MLAPM(version='GC', **{**LAW, **kw})


def test_runs_with_an_infinite_margin_members_and_captured_replays():
    """41 frames: scheduled passes at counter values 1, 9, 17, 25, 33"""
    from piml_amd import ops_scenario
    sc, nav = hall(), hall_field()
    never = ops_scenario.exit_choice_law([[1, 2]], margin=float('inf'))
    law = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)
    m = _mlapm(Aw=50.0, Bw=-5.0)
    plain = m.simulate_ensemble(sc, 41, [3, 4, 5], capacity=48, nav=nav, use_graph=False)
    assert plain.exit_switches is None
    idle = m.simulate_ensemble(sc, 41, [3, 4, 5], capacity=48, nav=nav, exit_choice=never, use_graph=False)
    assert _same(idle, plain) and torch.equal(idle.exit_gate, plain.exit_gate) and int(idle.exit_switches.sum()) == 0
    eager = m.simulate_ensemble(sc, 41, [3, 4, 5], capacity=48, nav=nav, exit_choice=law, use_graph=False)
    assert int(eager.exit_switches.sum()) >= 3 and not _same(eager, plain)
    assert tuple(eager.exit_gate.shape) == (3, 48) and eager.exit_gate.dtype == torch.int32
    captured = m.simulate_ensemble(sc, 41, [3, 4, 5], capacity=48, nav=nav, exit_choice=law, use_graph=True)
    assert _same(captured, eager) and torch.equal(captured.exit_gate, eager.exit_gate)
    assert torch.equal(captured.exit_switches, eager.exit_switches)
    one = m.simulate_scenario(sc, 41, seed=4, capacity=48, nav=nav, exit_choice=law)
    mem = eager.member(1)
    assert _same(mem, one) and torch.equal(mem.exit_gate, one.exit_gate) and torch.equal(mem.exit_switches, one.exit_switches)
    assert one.exit_counts() == eager.exit_counts()[1] and len(one.exit_counts()) == 3
    # True takes the scene's classes with the defaults; the density term composes
    default = m.simulate_scenario(sc, 41, seed=4, capacity=48, nav=nav, exit_choice=True)
    assert int(default.exit_switches.sum()) >= 1
    dense = m.simulate_ensemble(sc, 41, [3, 4], capacity=48, nav=nav, exit_choice=law, use_graph=True,
                                nav_density=ops_scenario.nav_density_law(2.0, every=8))
    assert int(dense.exit_switches.sum()) >= 1
    from piml_amd.models.mlapm import MLAPM
    sweep = MLAPM.simulate_sweep(sc, 41, [dict(version='GC', **LAW, Aw=50.0, Bw=-5.0)], [3, 4, 5], capacity=48, nav=nav,
                                 exit_choice=law, use_graph=False)
    assert _same(sweep, eager) and torch.equal(sweep.exit_switches, eager.exit_switches)


def test_network_driven_runs():
    """BaseSimulator.simulate_ensemble(..., exit_choice=): the choice launch between the network's forward and the frame, in the
    captured frame too.  An infinite margin is the run without the argument; a finite one switches agents and leaves the
    arrivals alone"""
    from piml_amd import ops_scenario
    from piml_amd.models.simulators import BaseSimulator
    from test_simulator_gpu import sim_args
    torch.manual_seed(0)
    sim = BaseSimulator(sim_args())
    sim.model.eval()
    sc, nav = hall(), hall_field()
    never = ops_scenario.exit_choice_law([[1, 2]], margin=float('inf'))
    law = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)
    plain = sim.simulate_ensemble(sc, 30, [3, 4], capacity=48, nav=nav)
    idle = sim.simulate_ensemble(sc, 30, [3, 4], capacity=48, nav=nav, exit_choice=never)
    assert _same(idle, plain) and torch.equal(idle.exit_gate, plain.exit_gate) and int(idle.exit_switches.sum()) == 0
    eager = sim.simulate_ensemble(sc, 30, [3, 4], capacity=48, nav=nav, exit_choice=law, use_graph=False)
    captured = sim.simulate_ensemble(sc, 30, [3, 4], capacity=48, nav=nav, exit_choice=law, use_graph=True)
    assert int(eager.exit_switches.sum()) >= 2 and torch.equal(eager.spawn_count, plain.spawn_count)
    assert torch.equal(captured.exit_switches, eager.exit_switches) and torch.equal(captured.exit_gate, eager.exit_gate)
    assert torch.equal(bits(captured.waypoints), bits(eager.waypoints))


def test_nearer_exit():
    """(a) one room, the entrance A on the left wall, the near exit on the bottom wall 5 m from it, the far exit on the right
    wall 19 m away; pair forces off, the wall term on, no noise.  Every agent that entered at A and retired left through the
    gate the restatement names at its spawn cell; without the choice some leave through the other."""
    from piml_amd import ops_scenario
    sc, nav = hall(6, 2.0), hall_field()
    law = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=2.0, every=8)
    m = _mlapm(A=0.0, Aw=50.0, Bw=-5.0)
    T, cap, seed = 330, 96, 1
    res = m.simulate_scenario(sc, T, seed=seed, capacity=cap, nav=nav, exit_choice=law)
    plain = m.simulate_scenario(sc, T, seed=seed, capacity=cap, nav=nav)
    n = res.num_agents
    import scenario_ref
    ent = sc.entries.cpu().numpy()
    dr = scenario_ref.agent_draws(seed, np.arange(n), ent.shape[0], ent.shape[1])
    u = nav.u.cpu().numpy()
    cls = REF.gate_class(law.classes, 3)
    first = res.mask_p[:, :n].argmax(0).cpu().numpy()            # the frame each agent appears in
    p0 = res.position[:, :n].cpu().numpy()[first, np.arange(n)]
    retired = (res.mask_p[-1, :n] == 0).cpu().numpy()
    retired_plain = (plain.mask_p[-1, :n] == 0).cpu().numpy()
    gate, old = res.exit_gate[:n].cpu().numpy(), plain.exit_gate[:n].cpu().numpy()
    margin = REF.cells(law.margin, nav.cell)
    judged = left_out = other = 0
    for i in np.flatnonzero((dr['oe'] == 0) & retired):
        cx, cy = REF.cell_of(p0[i], nav.x0, nav.y0, nav.cell, nav.gx, nav.gy)
        col = u[:, cy, cx]
        if abs(float(col[1]) - float(col[2])) < float(margin) + 2.0:
            left_out += 1
            continue
        named = REF.decide(u, (cx, cy), cls, int(dr['de'][i]), 0, margin, f32(0))
        named = int(dr['de'][i]) if named is None else named
        judged += 1
        assert gate[i] == named, (i, gate[i], named, col)
        other += int(old[i] != named and retired_plain[i])
    print(f'\n[navchoice] nearer exit: {n} agents, {judged} judged, {left_out} left out, {other} left by the other gate without '
          f'the choice; exits per gate {res.exit_counts()} against {plain.exit_counts()}')
    assert judged >= 8 and left_out <= (judged + left_out) / 4
    assert other >= 1
    assert torch.equal(plain.spawn_count, res.spawn_count)      # the arrivals do not depend on the choice


def test_queue_at_the_near_exit():
    """(b) the two-door prototype of tests/test_navdensity.py with the doors as the two exits of one class: 25 agents queued at
    the near door.  After one nav_field_update and one choice pass the probes standing clear of the queue are bound for the
    far exit with kd = 2 and for the near one with kd = 0, as the restatement says on the restated field"""
    from piml_amd import ops_scenario
    blocked, _, _ = navcost_ref.two_door_case()
    gy, gx = blocked.shape
    cell, wall = navcost_ref.TWO_DOOR_CELL, navcost_ref.TWO_DOOR_WALL
    goal = np.zeros((3, gy, gx), np.uint8)
    goal[0, 12, 2] = 1
    goal[1, list(navcost_ref.NEAR_DOOR), wall] = 1
    goal[2, list(navcost_ref.FAR_DOOR), wall] = 1
    centre = lambda x, y: (f32((x + 0.5) * cell), f32((y + 0.5) * cell))
    entries = np.array([[centre(2, 12)] * 3, [centre(wall, y) for y in navcost_ref.NEAR_DOOR],
                        [centre(wall, y) for y in navcost_ref.FAR_DOOR]], f32)
    probes = [(5, 11), (5, 12), (10, 9), (10, 12), (5, 5)]       # clear of the queue, nearer the near door
    cap, seed = 64, 2
    import scenario_ref
    oe = scenario_ref.agent_draws(seed, np.arange(cap), 3, 3)['oe']
    slots = np.flatnonzero(oe == 0)[:len(probes)]                # probes came in through gate 0: both exits are candidates
    rest = [i for i in range(cap) if i not in set(slots.tolist())][:25]
    s = dict(p=np.full((cap, 2), np.nan, f32), dest=np.full((cap, 2), np.nan, f32), flag=np.zeros(cap, np.int32),
             mask=np.zeros(cap, f32), waypoints=np.full((2, cap, 2), np.nan, f32), exit_idx=np.ones((2, cap), np.int32), n=cap)
    s['p'][rest] = navcost_ref.two_door_positions()
    s['p'][slots] = [centre(*c) for c in probes]
    live = np.concatenate([slots, rest])
    s['mask'][live] = 1
    s['dest'][live] = s['waypoints'][:, live] = entries[1, 1]
    law = ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=2.0, every=8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    u0, _ = navcost_ref.solve(blocked, goal, np.ones((gy, gx), f32))
    base = ops_scenario.NavField(dev(u0), dev(blocked), dev(goal), 0.0, 0.0, cell, 2.0)
    bound = {}
    for kd in (2.0, 0.0):
        st = ops_scenario.scenario_state(_scenario(entries, num_waypoints=2), cap, 4, seed=seed)
        _put(st, [s], 9)
        field = ops_scenario.NavFieldDynamic(base, 1)
        dlaw = ops_scenario.nav_density_law(kd, rho0=0.5, radius=cell, fmax=8.0, every=8)
        ops_scenario.nav_field_update(field, st, dlaw)
        count = navcost_ref.deposit(s['p'][None], s['mask'][None], 0.0, 0.0, cell, gx, gy)
        f, _ = navcost_ref.cost(count, cell, 1, kd, 0.5, 8.0)
        u, _ = navcost_ref.solve(blocked, goal, f[0])
        assert np.array_equal(field.u[0].cpu().numpy().view(np.uint32), u.view(np.uint32))
        want, switched = REF.choose(s, u, 0.0, 0.0, cell, REF.gate_class(law.classes, 3), REF.cells(1.0, cell), REF.cells(2.0, cell),
                                    8, 9, seed, entries, CASES.SPAWN_OFFSET)
        before = _snapshot(st)
        ops_scenario.nav_choose_exit(st, field, law)
        _assert_state(st, before, [want], kd)
        bound[kd] = st.exit_idx[0, dev(slots)].cpu().tolist()
        assert bound[kd] == want['exit_idx'][0, slots].tolist()
    assert bound[2.0] == [2] * len(probes) and bound[0.0] == [1] * len(probes)


# ---- 4. the command line ----

def test_command_line_run_reports_the_exits(tmp_path):
    from piml_amd.trackstats import TrackStats
    plan, out = tmp_path / 'plan.json', str(tmp_path / 'track.json')
    plan.write_text(json.dumps(dict(walls=HALL_WALLS, gates=HALL_GATES, exits=[[1, 2]], n_initial=10, rate_per_s=2.0,
                                    arrival_radius=0.5, spawn_offset=0.4)))
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scene-plan', str(plan), '--nav', '--nav-cell',
                        '0.5', '--exit-choice', '--exit-commit', '1', '--seeds', '3:5', '--frames', '120', '--track-stats', out],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert '[simulate] exit choice: exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)' in p.stdout
    assert p.stdout.count('exits per gate') == 2
    got = json.load(open(out))
    counts = got['exit_counts']
    assert len(counts) == 2 and all(len(c) == 3 for c in counts) and sum(map(sum, counts)) >= 4 and got['exit_switches'] >= 1
    TrackStats.from_json(out)                                    # the statistics' own reader takes the file as before
