"""GPU: the MLAPM scenario frame routed by the floor field (piml_scenario_step_mlapm_nav; MLAPM.simulate_*(..., nav=)).  A
field that is +inf everywhere is the run without the field, bit for bit; the first frame of a small plan is the existing frame
on a state whose destinations were overwritten by p + e of ops_scenario.nav_direction; the arrivals do not depend on the field;
members, table forms and captured replays are bitwise each other; and in two rooms joined by a door every agent goes through
the door with the field and through the wall without it."""
import dataclasses
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_scenario_mlapm_gpu import FIELDS, LAW, _same, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = [0, 1, 2]
PLAIN = dict(version='GC', **LAW)
WALLED = dict(PLAIN, Aw=50.0, Bw=-5.0)
NOISY = dict(WALLED, An=0.5, noise_tau=0.5)
# two rooms and a door: gates at x = 0 and x = 10 over y in [0.5, 3]; a wall on x = 5 from below the grid to above it, open
# over y in (4.5, 5.5).  BOUNDS end inside the wall's extent: a wall that ends inside the grid gets walked around
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
    kw = dict(n_initial=12, rate_per_s=2.0, arrival_radius=0.5) if name == 'plan' else dict(n_initial=10, rate_per_s=1.2)
    return scenarios.floorplan_scenario(WALLS, GATES, **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def field(name):
    from piml_amd import ops_scenario
    if name == 'inf':                                            # 8 x 8 cells of 5 m over GC's hall: every lookup is branch 0
        u = torch.full((7, 8, 8), float('inf'), device=DEV)
        z = torch.zeros(7, 8, 8, dtype=torch.uint8, device=DEV)
        return ops_scenario.NavField(u, z[0].clone(), z, 0.0, 0.0, 5.0, 2.0)
    return ops_scenario.nav_field(scene(name), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV)


# ---- 1. nothing but e moved ----

@pytest.mark.parametrize('params', [PLAIN, WALLED, NOISY], ids=['plain', 'walls', 'walls+noise'])
def test_infinite_field_is_the_run_without_one(params):
    """single, members and table forms on GC with route_max_iters = 0, 40 frames: the reference run is the entries the parent
    commit had (piml_scenario_step_mlapm / _laws / _walls / _noise), not the new one"""
    sc, nav = scene('gc'), field('inf')
    sim = MLAPM(**params)
    without = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP)
    assert sum(without.spawned) > 3 * 20 and float(without.mask_p[:, -1].sum()) > 30
    with_ = sim.simulate_ensemble(sc, 40, SEEDS, capacity=CAP, nav=nav)
    assert all(_same(with_.member(m), without.member(m)) for m in range(len(SEEDS)))
    one = sim.simulate_scenario(sc, 40, seed=SEEDS[1], capacity=CAP, nav=nav)
    assert _same(one, without.member(1))
    table = sim.simulate_sweep(sc, 40, [params], SEEDS, capacity=CAP, nav=nav)
    assert all(_same(table.member(m), without.member(m)) for m in range(len(SEEDS)))


# ---- 2. the first frame ----

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
def test_first_frame_is_the_existing_frame_steered_to_p_plus_e(params):
    """v' and a' of the frame with the field == the existing frame's on a state whose destination is p + e_nav (the lookup's
    branches 1 and 2; branch 0 keeps its destination), bitwise -- the tolerance of
    test_scenario_walls_gpu.py::test_first_frame_adds_the_operators_wall_force -- for the agents that arrived nowhere"""
    from piml_amd import ops_scenario
    nav = field('plan')
    seen = {}

    def overwrite(st):
        gate = torch.gather(st.exit_idx, 1, st.flag.long().unsqueeze(1)).squeeze(1)        # exit_idx[flag]: (S, cap)
        e, b, _ = ops_scenario.nav_direction(st.p, gate, st.dest, nav, return_branch=True)
        seen.update(p=st.p.clone(), b=b, present=st.mask == 1)
        st.dest.copy_(torch.where((b > 0).unsqueeze(-1), st.p + e, st.dest))
    got = _first_frame(params, nav)
    want = _first_frame(params, None, overwrite)
    plain = _first_frame(params, None)
    assert torch.equal(bits(seen['p']), bits(plain.p_res[:, 0])) and int(seen['present'].sum()) == 3 * 12
    stayed = seen['present'] & (got.mask == 1) & (want.mask == 1) & (got.flag == 0) & (want.flag == 0)
    routed = stayed & (seen['b'] > 0)
    print(f'\n[nav] first frame: {int(seen["present"].sum())} agents, {int(stayed.sum())} arrived nowhere, branches '
          f'{torch.bincount(seen["b"][seen["present"]].long(), minlength=3).tolist()}')
    assert int(routed.sum()) >= 24                               # the field routes most of them (their gate is far)
    for k in ('v', 'a', 'p'):
        assert torch.equal(bits(getattr(got, k)[stayed]), bits(getattr(want, k)[stayed])), k
    assert not torch.equal(bits(got.v[routed]), bits(plain.v[routed]))           # ... and e did move
    assert torch.equal(bits(got.v[stayed & ~routed]), bits(plain.v[stayed & ~routed]))
    # v' = v + F dt, p' = p + v' dt with the frame's force, as every frame
    dt = float(got.scenario.time_unit)
    assert torch.equal(bits(got.v[stayed]), bits((got.a * dt)[stayed]))          # (v = 0 at birth)
    assert torch.equal(bits(got.p[stayed]), bits((seen['p'] + got.v * dt)[stayed]))


# ---- 3. arrivals, forms ----

@functools.lru_cache(maxsize=None)
def plan_runs(routed):
    sim = MLAPM(**WALLED)
    return sim.simulate_ensemble(scene('plan'), 60, SEEDS, capacity=CAP, nav=field('plan') if routed else None)


def test_arrivals_do_not_depend_on_the_field():
    plain, routed = plan_runs(False), plan_runs(True)
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


def test_members_table_forms_and_captured_replay_are_bitwise_equal():
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    sc, nav, ens = scene('plan'), field('plan'), plan_runs(True)
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
    two = MLAPM(**PLAIN).simulate_sweep(sc, 60, [WALLED, dict(WALLED, tau=0.6)], SEEDS[:2], capacity=CAP, nav=nav)
    assert all(_same(two.member(m), ens.member(m)) for m in range(2))           # candidates share the scene's field
    assert not _same(two.member(2), ens.member(0))


# ---- 4. two rooms and a door ----

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
    """pair forces off (A = 0): the outcome is the field's.  400 frames of dt = 0.08, tau = 0.5, cell 0.25, clearance 0.3."""
    law = dict(PLAIN, A=0.0, tau=0.5)
    sc, nav = scene('rooms'), field('rooms')
    assert float(sc.time_unit) == 0.08 and (nav.cell, nav.clearance) == (0.25, 0.3)
    # the wall spans the whole grid height but for the door
    col = nav.blocked[:, int((5.0 - nav.x0) / 0.25)].cpu().numpy()
    rows_y = nav.y0 + (np.arange(nav.gy) + 0.5) * 0.25
    assert col[(rows_y < 4.5) | (rows_y > 5.5)].all() and not col[(rows_y > 4.85) & (rows_y < 5.15)].any()
    routed = MLAPM(**law).simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP, nav=nav)
    straight = MLAPM(**law).simulate_ensemble(sc, 400, SEEDS[:2], capacity=CAP)
    assert routed.dropped == [0, 0] and min(routed.spawned) >= 30
    y, agents = _crossings(routed)
    obs = sc.obstacles.cpu().numpy().astype(np.float64)
    pos = routed.position.cpu().numpy().astype(np.float64)[routed.mask_p.cpu().numpy() == 1]
    closest = min(float(np.sqrt(((obs - q) ** 2).sum(1).min())) for q in pos[::7])
    print(f'\n[nav] two rooms, with the field: {y.size} steps across x = 5 by {agents} agents, y in [{y.min():.3f}, {y.max():.3f}], '
          f'closest approach to the wall {closest:.3f} m (every 7th position)')
    assert y.size >= 40 and ((y > 4.5) & (y < 5.5)).all()        # no recorded step crosses x = 5 outside the door
    m = routed.mask_p.cpu().numpy()
    early = (m[:, :100] == 1).any(1)                             # spawned in the first 100 frames ...
    assert early.sum() >= 2 * 12 and (m[:, -1][early] == 0).all()                # ... and retired by the end
    y0, agents0 = _crossings(straight)
    print(f'[nav] two rooms, without: {y0.size} steps across x = 5 by {agents0} agents, y in [{y0.min():.3f}, {y0.max():.3f}]')
    assert y0.size >= 40 and ((y0 < 4.5) | (y0 > 5.5)).all()     # every agent that reaches x = 5 crosses it through the wall


# ---- 5. errors and the command line ----

def test_errors_and_the_command_line(tmp_path):
    from piml_amd import ops_scenario, scenarios
    sc, nav = scene('plan'), field('plan')
    st = scenarios.scenario_state_for(scenarios.gc_scenario(), 4, 32, DEV, seeds=SEEDS)           # route_max_iters = 16
    ops_scenario.scenario_step(st, init=True)
    law = ops_scenario.mlapm_law()
    with pytest.raises(ValueError, match='route_max_iters'):
        ops_scenario.scenario_step_mlapm(st, law, nav=field('inf'))
    st = scenarios.scenario_state_for(scene('gc'), 4, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st, init=True)
    with pytest.raises(ValueError, match='gates'):
        ops_scenario.scenario_step_mlapm(st, law, nav=nav)       # 2 gates for a scene of 7
    with pytest.raises(TypeError):
        ops_scenario.scenario_step_mlapm(st, law, nav=True)
    st2 = scenarios.scenario_state_for(scenarios.crosswalk_scenario(), 4, 32, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st2, init=True)
    with pytest.raises(ValueError, match='gates'):
        ops_scenario.scenario_step_mlapm(st2, law, nav=nav)
    assert int(st.t.item()) == 0 and int(st2.t.item()) == 0
    with pytest.raises(ValueError, match='route_max_iters'):
        MLAPM(**PLAIN).simulate_scenario(scenarios.gc_scenario().to(DEV), 5, nav=True)
    # the entry's own refusals, with descriptors that pass but for the one thing
    from piml_amd import _lib
    import ctypes
    call = lambda s, navd: _lib.lib().piml_scenario_step_mlapm_nav(
        ctypes.byref(s), ctypes.byref(st.rules), 3, st.seeds.data_ptr(), ctypes.byref(law), None, None, None, None,
        ctypes.byref(navd), None, 0, None)
    iters = _lib.Scenario.from_buffer_copy(st.desc)
    iters.route_max_iters = 1
    wrong = _lib.NavGrid.from_buffer_copy(field('inf').desc)
    wrong.G = 6
    assert call(iters, field('inf').desc) == 1 and call(st.desc, wrong) == 1
    assert call(st.desc, field('inf').desc) == 0                 # the argument set every refusal test differs from
    torch.cuda.synchronize()
    # nav=True builds the scene's field with the defaults
    auto = MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=True)
    default = ops_scenario.nav_field(sc, device=DEV)
    assert _same(auto, MLAPM(**PLAIN).simulate_scenario(sc, 20, seed=1, capacity=CAP, nav=default))
    # the command line on a plan file
    plan = tmp_path / 'plan.json'
    plan.write_text(json.dumps(dict(walls=WALLS, gates=GATES, n_initial=12, rate_per_s=2.0, arrival_radius=0.5)))
    out = tmp_path / 'walls.json'
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scene-plan', str(plan), '--nav',
                        '--frames', '60', '--seeds', '0:2', '--capacity', str(CAP), '--obstacle-stats', str(out)], cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'floor field: 2 gates' in p.stdout
    from piml_amd.obstaclestats import ADDITIVE, ObstacleStats
    got = ObstacleStats.from_json(str(out))
    want = MLAPM(**PLAIN).simulate_ensemble(sc, 60, [0, 1], capacity=CAP, nav=default).obstacle_stats()
    assert all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ADDITIVE)
    plain = MLAPM(**PLAIN).simulate_ensemble(sc, 60, [0, 1], capacity=CAP).obstacle_stats()
    assert not all(np.array_equal(getattr(plain, k), getattr(want, k)) for k in ADDITIVE)       # the field ran
