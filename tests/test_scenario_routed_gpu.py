"""GPU: the network-driven scenario frame routed by the floor field (piml_scenario_step_nav; ops_scenario.scenario_step(nav=),
BaseSimulator.simulate_*(..., nav=), simulate --route).  There is no routing in the reference; the oracles are two things this
repository pins bit for bit elsewhere -- ops_scenario.nav_direction (tests/nav_ref.py) and the unrouted scenario_step
(tests/scenario_ref.py) -- and every comparison below is the same inline function on the same inputs or code that did not
change, so it is bitwise.  Frame by frame a routed state is its unrouted twin plus steer = p + e of the lookup; the steering
target reaches the network as its destination feature and nothing else moves; arrivals do not depend on the field; and in two
rooms joined by a door a network reduced to its desired-force term goes through the door with the field and through the wall
without it.  Scene constants are test_scenario_nav_gpu.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_scenario_ensemble_gpu import _row_invariant
from test_scenario_mlapm_gpu import _same, bits
from test_scenario_nav_gpu import CAP, GATES, SEEDS, WALLS, _crossings, field, scene
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STATE = ('p', 'v', 'a', 'dest', 'flag', 'mask', 'waypoints', 'exit_idx', 'desired_speed', 'hist', 'spawned', 'spawn_count',
         'dropped', 'p_res', 'v_res', 'a_res', 'dest_res', 'mask_res')


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


def _member_is_the_single_run(sim, ens, m, one):
    """Member m of an ensemble against the single run of its seed, by the rule of
    test_scenario_ensemble_gpu.py::test_simulate_ensemble_end_to_end: bitwise where the network gives a row the
    same bits among S * capacity rows as among capacity; otherwise the arrivals bitwise and frames 0 .. 1 (the network's first
    output) within 1e-6 -- the row count is the network's business, not the frame's."""
    mem = ens.member(m)
    if _row_invariant(sim, ens):
        return _same(mem, one)
    for k in ('position', 'velocity', 'acceleration'):
        x, y = getattr(mem, k)[:2], getattr(one, k)[:2]
        if not torch.equal(x.isnan(), y.isnan()) or (torch.nan_to_num(x) - torch.nan_to_num(y)).abs().max().item() > 1e-6:
            return False
    return mem.spawned == one.spawned and mem.dropped == one.dropped and all(
        torch.equal(bits(getattr(mem, k)), bits(getattr(one, k))) for k in ('waypoints', 'desired_speed', 'spawn_count'))


def sight_field(name):
    from piml_amd import ops_scenario
    from test_scenario_nav_gpu import BOUNDS
    return ops_scenario.nav_field(scene(name), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV, sight=True)


def _gate(st):
    """exit_idx[flag] of every slot (a retired slot's flag may be D: clamped, its row is not compared)"""
    D = st.exit_idx.shape[-2]
    return torch.gather(st.exit_idx, -2, st.flag.clamp(max=D - 1).long().unsqueeze(-2)).squeeze(-2)


def _want_steer(st, nav):
    """(where(b > 0, p + e, dest), b) of the lookup on st's state"""
    from piml_amd import ops_scenario
    e, b, _ = ops_scenario.nav_direction(st.p, _gate(st), st.dest, nav, return_branch=True)
    return torch.where((b > 0).unsqueeze(-1), st.p + e, st.dest), b


def _twins(sc, nav, T, cap, seeds):
    """Twin A stepped by scenario_step(nav=), twin B without; both take a_next = (v0 e - v) / 0.5 with e the unit vector of A's
    routed destination features, so the agents follow the field.  After every frame: every state tensor and record of A is
    bitwise B's, and A.steer is the lookup on B's state for mask == 1 and NaN elsewhere.  Returns (A, B, ok (T, len(STATE) + 1)
    bool on the host, branch counts (T, 4) of the live slots)."""
    from piml_amd import ops, ops_scenario, scenarios
    A = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=seeds)
    B = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=seeds)
    feats = (A.pf, A.of, A.selff, A.ped_idx, A.obs_idx)
    ok, branches = [], []

    def look():
        same = [(bits(getattr(A, k)) == bits(getattr(B, k))).all() for k in STATE]
        want, b = _want_steer(B, nav)
        live = B.mask == 1
        same.append(torch.where(live.unsqueeze(-1), bits(A.steer) == bits(want), A.steer.isnan()).all())
        ok.append(torch.stack(same))
        branches.append(torch.bincount(b[live].long(), minlength=4)[:4])
    ops_scenario.scenario_step(A, init=True, nav=nav)
    ops_scenario.scenario_step(B, init=True)
    look()
    for _ in range(T - 1):
        ops.relative_features_into(feats, A.p, A.v, A.a, A.steer, sc.obstacles)
        d = A.selff[..., :2]
        e = torch.nan_to_num(d / d.norm(dim=-1, keepdim=True))
        a_next = ((A.desired_speed.unsqueeze(-1) * e - A.v) / 0.5).contiguous()
        ops_scenario.scenario_step(A, a_next, nav=nav)
        ops_scenario.scenario_step(B, a_next)
        A.t.add_(1)
        B.t.add_(1)
        look()
    torch.cuda.synchronize()
    return A, B, torch.stack(ok).cpu().numpy(), torch.stack(branches).cpu().numpy()


def _assert_twins(ok):
    names = STATE + ('steer',)
    bad = np.argwhere(~ok)
    assert bad.size == 0, f'first difference at frame {bad[0][0]}: {names[bad[0][1]]}; in all: {sorted({names[j] for _, j in bad})}'


# ---- 1. frame by frame against a twin ----

@pytest.mark.parametrize('table', [False, True], ids=['field', 'field+table'])
def test_frame_by_frame_the_routed_state_is_its_twin_plus_steer(table):
    sc = scene('plan')
    nav = sight_field('plan') if table else field('plan')
    T = 200
    A, B, ok, branches = _twins(sc, nav, T, CAP, SEEDS)
    n = torch.minimum(A.spawned[:, (T - 1) & 1], torch.tensor(CAP, device=DEV))
    retired = ((torch.arange(CAP, device=DEV)[None] < n[:, None]) & (A.mask == 0)).sum(1).tolist()
    later = A.spawn_count[:, 1:].sum(1).tolist()
    print(f'\n[routed] plan, {"table" if table else "field"}: frame 0 branches {branches[0].tolist()}, over {T} frames '
          f'{branches.sum(0).tolist()}; spawned after frame 0 {later}, retired {retired}, dropped {A.dropped.tolist()}')
    _assert_twins(ok)
    assert int(branches[0].sum()) == 3 * 12 and int(branches[0][1:].sum()) >= 24       # the field routes most of them
    assert min(later) >= 1 and min(retired) >= 1                 # every member spawned after frame 0 and retired an agent
    assert (int(branches[:, 3].sum()) >= 1) == table             # the table's branch, and only with the table


# ---- 2. the second agent block ----

def test_second_agent_block():
    """280 initial agents in 300 slots: slots 256 .. 279 are live in a partial second block of 256 threads"""
    from piml_amd import scenarios
    sc = scenarios.floorplan_scenario(WALLS, GATES, n_initial=280, rate_per_s=2.0, arrival_radius=0.5).to(DEV)
    A, B, ok, branches = _twins(sc, field('plan'), 7, 300, [5])
    _assert_twins(ok)
    assert int(branches[0].sum()) == 280 and int(branches[-1].sum()) >= 256 + 20
    assert (B.mask_res[0, 0, 256:280] == 1).all() and (B.mask_res[0, 0, 280:] == 0).all()
    tail = A.steer[0, 256:280][A.mask[0, 256:280] == 1]
    assert tail.shape[0] >= 20 and not tail.isnan().any()


# ---- 3. canary ----

def test_small_capacity_writes_no_steer_past_it_and_drops_the_unrouted_ordinals():
    """buffers of 32 slots, desc.capacity = 24 (test_scenario_gpu.py::test_small_capacity_drops_exactly_the_restatements_ordinals)"""
    from piml_amd import ops_scenario
    sc, nav = scene('gc'), field('inf')
    seed, T, cap, pad = 3, 200, 24, 32
    runs = []
    for routed in (True, False):
        st = ops_scenario.scenario_state(sc, pad, T, seed=seed)
        st.desc.capacity = cap
        kw = {}
        if routed:
            st.steer = torch.full((pad, 2), 12345.0, device=DEV)
            kw = dict(nav=nav)
        ops_scenario.scenario_step(st, init=True, **kw)
        for _ in range(T - 1):
            ops_scenario.scenario_step(st, torch.zeros(pad, 2, device=DEV), **kw)
            st.t.add_(1)
        runs.append(st)
    torch.cuda.synchronize()
    A, B = runs
    assert (A.steer[cap:] == 12345.0).all() and not (A.steer[:cap] == 12345.0).any()     # every slot below was written, none above
    total = int(B.spawned[(T - 1) & 1].item())
    assert total > cap and int(A.spawned[(T - 1) & 1].item()) == total
    assert int(A.dropped.item()) == int(B.dropped.item()) == total - cap
    assert torch.equal(A.spawn_count, B.spawn_count)
    for k in ('p', 'v', 'mask', 'flag', 'p_res', 'mask_res', 'waypoints', 'exit_idx', 'dest_res'):
        assert torch.equal(bits(getattr(A, k)), bits(getattr(B, k))), k      # the canary tails included
    live = A.mask.reshape(-1)[:cap] == 1
    assert torch.equal(bits(A.steer[:cap][live]), bits(A.dest[:cap][live]))     # branch 0


# ---- 4. an infinite field is the run without one ----

def test_infinite_field_is_the_run_without_one(sim):
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    sc, nav = scene('gc'), field('inf')
    without = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP)
    assert sum(without.spawned) > 3 * 20 and float(without.mask_p[:, -1].sum()) > 30
    with_ = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=nav)
    assert all(_same(with_.member(m), without.member(m)) for m in range(len(SEEDS)))
    one = sim.simulate_scenario(sc, 40, seed=SEEDS[1], capacity=CAP, nav=nav)
    assert _same(one, sim.simulate_scenario(sc, 40, seed=SEEDS[1], capacity=CAP))         # the single run, bit for bit
    assert _member_is_the_single_run(sim, without, 1, one)
    graph = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=nav, use_graph=True)
    eager = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=nav, use_graph=False)
    assert all(_same(graph.member(m), eager.member(m)) and _same(graph.member(m), without.member(m)) for m in range(len(SEEDS)))
    live = with_.state.mask == 1
    assert torch.equal(bits(with_.state.steer[live]), bits(with_.state.dest[live])) and with_.state.steer[~live].isnan().all()


# ---- 5. the network sees the target ----

@pytest.mark.parametrize('T', [1, 9, 40])
def test_the_network_sees_the_target(sim, T):
    from piml_amd import ops
    sc, nav = scene('plan'), field('plan')
    a = sim.args
    geo = (a.topk_ped, a.sight_angle_ped, a.dist_threshold_ped, a.topk_obs, a.sight_angle_obs, a.dist_threshold_obs)
    res = sim.simulate_scenario(sc, T, seed=SEEDS[1], capacity=CAP, use_graph=False, nav=nav)
    st = res.state
    last = (res.position[T - 1], res.velocity[T - 1], res.acceleration[T - 1])
    assert torch.equal(bits(last[0]), bits(st.p)) and torch.equal(bits(res.destination[T - 1]), bits(st.dest))
    with torch.no_grad():
        pf, of, df = ops.relative_features(*last, st.steer, sc.obstacles, *geo)
        pf0, of0, df0 = ops.relative_features(*last, res.destination[T - 1], sc.obstacles, *geo)
    assert torch.equal(bits(st.selff[:, :2]), bits(df))          # the target reached the network as its destination feature
    for got, x, y in ((st.pf, pf, pf0), (st.of, of, of0)):       # the neighbour features do not depend on the destination
        assert torch.equal(bits(got), bits(x)) and torch.equal(bits(got), bits(y))
    want, b = _want_steer(st, nav)
    routed = (st.mask == 1) & (b > 0)
    assert int(routed.sum()) >= 4                                # (a third of the 12 initial agents; the three-member count is 24 of 36)
    assert (bits(st.selff[:, :2])[routed] != bits(df0)[routed]).any(1).all()     # every routed agent is steered elsewhere
    straight = (st.mask == 1) & (b == 0)
    assert torch.equal(bits(st.selff[:, :2][straight]), bits(df0[straight]))
    assert torch.equal(bits(st.steer[st.mask == 1]), bits(want[st.mask == 1])) and st.steer[st.mask == 0].isnan().all()


# ---- 6. arrivals do not depend on the field ----

def test_arrivals_do_not_depend_on_the_field(sim):
    sc, nav = scene('plan'), field('plan')
    plain = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP)
    routed = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav)
    assert routed.spawned == plain.spawned and routed.dropped == plain.dropped and sum(plain.spawned) > 3 * 12
    for k in ('spawn_count', 'desired_speed', 'waypoints'):
        assert torch.equal(bits(getattr(routed, k)), bits(getattr(plain, k))), k
    assert torch.equal(routed.state.exit_idx, plain.state.exit_idx)
    born = torch.zeros_like(plain.mask_p, dtype=torch.bool)
    born[:, 0] = plain.mask_p[:, 0] == 1
    born[:, 1:] = (plain.mask_p[:, 1:] == 1) & (plain.mask_p[:, :-1] == 0)
    assert torch.equal(bits(routed.position[born]), bits(plain.position[born])) and int(born.sum()) >= sum(
        min(n, plain.capacity) for n in plain.spawned)
    assert not torch.equal(bits(routed.position), bits(plain.position))
    for m, s in enumerate(SEEDS):                                # member m of a routed ensemble is the routed single run
        assert _member_is_the_single_run(sim, routed, m, sim.simulate_scenario(sc, 60, seed=s, capacity=CAP, nav=nav)), m
    graph = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav, use_graph=True)
    eager = sim.simulate_ensemble(sc, 60, SEEDS, capacity=CAP, nav=nav, use_graph=False)
    assert all(_same(graph.member(m), eager.member(m)) and _same(graph.member(m), routed.member(m)) for m in range(len(SEEDS)))
    assert torch.equal(bits(graph.state.steer), bits(eager.state.steer))


# ---- 7. two rooms and a door, under the network ----

def test_two_rooms_and_a_door_under_the_network():
    """pinnsf_m with tau = 0.5 and the last layers of both predictors zeroed: the output is the desired-force term alone, so the
    outcome is the field's.  400 frames of dt = 0.08, cell 0.25, clearance 0.3.  A CPU prototype of this frame (nav_ref.py's
    field and lookup, the lagged Euler, numpy arrivals) crossed 42 - 48 times per seed at y in 4.82 .. 5.26, never outside."""
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    s.model.tau = 0.5
    with torch.no_grad():
        for head in (s.model.ped_predictor, s.model.obs_predictor):
            last = [m for m in head.modules() if isinstance(m, torch.nn.Linear)][-1]
            last.weight.zero_()
            last.bias.zero_()
    sc, nav = scene('rooms'), field('rooms')
    assert float(sc.time_unit) == 0.08 and (nav.cell, nav.clearance) == (0.25, 0.3)
    routed = s.simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP, nav=nav)
    straight = s.simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP)
    assert routed.dropped == [0, 0] and min(routed.spawned) >= 30
    y, agents = _crossings(routed)
    print(f'\n[routed] two rooms under the network, with the field: {y.size} steps across x = 5 by {agents} agents, y in '
          f'[{y.min():.3f}, {y.max():.3f}]')
    assert y.size >= 40 and ((y > 4.5) & (y < 5.5)).all()        # no recorded step crosses x = 5 outside the door
    m = routed.mask_p.cpu().numpy()
    early = (m[:, :100] == 1).any(1)                             # present in the first 100 frames ...
    assert early.sum() >= 2 * 10 and (m[:, -1][early] == 0).all()                # ... and retired by the end
    y0, agents0 = _crossings(straight)
    print(f'[routed] two rooms under the network, without: {y0.size} steps across x = 5 by {agents0} agents, y in '
          f'[{y0.min():.3f}, {y0.max():.3f}]')
    assert y0.size >= 1 and ((y0 < 4.5) | (y0 > 5.5)).all()      # every crossing goes through the wall


# ---- 8. errors and the command line ----

def test_errors_and_the_command_line(sim, tmp_path):
    from piml_amd import ops_scenario, scenarios
    sc, nav = scene('plan'), field('plan')
    st = scenarios.scenario_state_for(scenarios.gc_scenario().to(DEV), 4, 32, DEV, seeds=SEEDS)          # route_max_iters = 16
    ops_scenario.scenario_step(st, init=True)
    a_next = torch.zeros_like(st.p)
    with pytest.raises(ValueError, match='route_max_iters'):
        ops_scenario.scenario_step(st, a_next, nav=field('inf'))
    st1 = scenarios.scenario_state_for(scene('gc'), 4, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st1, init=True)
    with pytest.raises(ValueError, match='gates'):
        ops_scenario.scenario_step(st1, a_next, nav=nav)         # 2 gates for a scene of 7
    with pytest.raises(TypeError):
        ops_scenario.scenario_step(st1, a_next, nav=True)
    st2 = scenarios.scenario_state_for(scenarios.crosswalk_scenario().to(DEV), 4, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st2, init=True)
    with pytest.raises(ValueError, match='gates'):
        ops_scenario.scenario_step(st2, a_next, nav=nav)
    assert int(st.t.item()) == 0 and int(st1.t.item()) == 0 and int(st2.t.item()) == 0
    assert st.steer is None and st1.steer is None and st2.steer is None          # nothing was allocated either
    with pytest.raises(ValueError, match='route_max_iters'):
        sim.simulate_scenario(scenarios.gc_scenario().to(DEV), 5, nav=True)
    # the argument set the refusals of test_scenario_routed.py differ from, and the seedless single run
    from piml_amd import _lib
    import ctypes
    one = ops_scenario.scenario_state(scene('gc'), 32, 4, seed=SEEDS[1])
    two = ops_scenario.scenario_state(scene('gc'), 32, 4, seed=SEEDS[1])
    steer = torch.full((32, 2), float('nan'), device=DEV)
    inf = field('inf')
    assert _lib.lib().piml_scenario_step_nav(ctypes.byref(one.desc), None, 1, None, None, 1, ctypes.byref(inf.desc), None,
                                             steer.data_ptr(), None) == 0
    ops_scenario.scenario_step(two, init=True, nav=inf)
    torch.cuda.synchronize()
    assert torch.equal(bits(one.p), bits(two.p)) and torch.equal(bits(steer), bits(two.steer)) and int((one.mask == 1).sum()) == 20
    # scenario_state_reset refills steer
    ops_scenario.scenario_state_reset(two)
    assert two.steer.isnan().all()
    # nav=True builds the scene's field with the defaults
    auto = sim.simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=True)
    default = ops_scenario.nav_field(sc, device=DEV)
    assert _same(auto, sim.simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=default))
    assert not _same(auto, sim.simulate_scenario(sc, 20, seed=1, capacity=CAP))
    # the command line on a plan file, under the network law
    plan = tmp_path / 'plan.json'
    plan.write_text(json.dumps(dict(walls=WALLS, gates=GATES, n_initial=12, rate_per_s=2.0, arrival_radius=0.5)))
    out = tmp_path / 'walls.json'
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--scene-plan', str(plan), '--route', 'field', '--frames', '60',
                        '--seeds', '0:2', '--capacity', str(CAP), '--obstacle-stats', str(out)], cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'floor field: 2 gates' in p.stdout
    from piml_amd.obstaclestats import ObstacleStats
    got = ObstacleStats.from_json(str(out))
    assert got is not None and os.path.getsize(str(out)) > 0
