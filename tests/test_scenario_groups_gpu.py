"""GPU: group arrivals and the group cohesion term of the MLAPM scenario frame (PIML_SPAWN_CLIP_GROUPS,
piml_scenario_step_mlapm_groups, piml_group_force) on a hand-made track table -- E = 10 rows: a pair and a single in the
first frame, then Ua = 4 arrival units (not a power of two: the integer unit map), a triple, a pair and two singles; D = 2
with one NaN second waypoint --: spawns and bookkeeping bitwise the numpy restatement's (tests/scenario_groups_ref.py), the
operator on its edge cases, the frame's force against the operator, members / forms / captured replays / sweeps bitwise
each other, the planted groups found again by the group statistics, the recorded GC clip and the command line.

Seeds, chosen with the restatement on the CPU: 12 frames at 0.6 units per frame and capacity 20.  It gives 3 + 14 = 17 agents
in 9 units for seed 4 and 3 + 16 = 19 in 8 units for seed 2^63 + 4 (nothing dropped, every kind of unit drawn; the second
keeps the key's top bit set), and 3 + 30 = 33 for seed 11, whose first triple of frame 6 has its base at slot 18: two of its
members are written, the third and the 12 agents that follow are dropped (seeds 0 .. 10 and 2^63 + 1 .. 9 hold no unit that
straddles slot 20 apart from 2^63 + 2's pair at 19; test_seeds_are_what_the_docstring_says holds the restatement to this)."""
import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import scenario_groups_ref as R
from conftest import GOLDEN, REPO
from conftest import bits as nbits
from test_pairstats_gpu import GC_CLIP, _raw
from test_scenario_mlapm_gpu import FIELDS, LAW, _same, _step_fwd, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = [4, 11, (1 << 63) + 4]
DROPPING = 11                                                 # the seed whose run passes the capacity
NAN = float('nan')
N0, CAP, T, RATE = 3, 20, 12, 0.6
PLAIN = dict(version='GC', **LAW)
NO_PAIRS = dict(PLAIN, A=0.0)                                  # no pair repulsion: agents walk straight to their waypoints
AG, GDIST = 3.0, 0.25                                         # (a pair 0.8 m apart is 0.4 m from its centroid: felt at 0.25)
AW, BW, CUTOFF = 50.0, -5.0, 2.0
GROUP_FIELDS = ('group_first', 'group_size')


def table(gap=0.8):
    """(position, velocity, (desired speed, 0), waypoint 0, waypoint 1) per row.  The members of a unit walk side by side,
    `gap` (the first pair) or 0.8 m apart, at one speed towards parallel destinations hundreds of metres away."""
    rows = [
        [[0.0, 0.0], [1.25, 0.0], [1.25, 0.0], [200.0, 0.0], [210.0, 0.0]],              # 0, 1: the first frame's pair
        [[0.0, gap], [1.25, 0.0], [1.25, 0.0], [200.0, gap], [210.0, gap]],
        [[5.0, -10.0], [-1.0, 0.0], [1.0, 0.0], [-200.0, -10.0], [NAN, NAN]],             # 2: its single
        [[0.0, 20.0], [1.5, 0.0], [1.5, 0.0], [300.0, 20.0], [310.0, 20.0]],              # 3, 4, 5: a triple
        [[0.0, 20.8], [1.5, 0.0], [1.5, 0.0], [300.0, 20.8], [310.0, 20.8]],
        [[0.0, 21.6], [1.5, 0.0], [1.5, 0.0], [300.0, 21.6], [310.0, 21.6]],
        [[50.0, 40.0], [-1.125, 0.0], [1.125, 0.0], [-200.0, 40.0], [-210.0, 40.0]],      # 6, 7: a pair
        [[50.0, 40.8], [-1.125, 0.0], [1.125, 0.0], [-200.0, 40.8], [-210.0, 40.8]],
        [[0.0, 60.0], [0.0, 1.0], [1.0, 0.0], [0.0, 300.0], [0.0, 310.0]],                # 8, 9: singles
        [[30.0, -30.0], [0.75, 0.5], [0.9013878, 0.0], [300.0, 150.0], [310.0, 156.0]]]
    return np.array(rows, np.float32)


TABLE = table()
ROW_UNIT = np.array([[0, 2], [1, 2], [0, 1], [0, 3], [1, 3], [2, 3], [0, 2], [1, 2], [0, 1], [0, 1]], np.int32)
UNIT_ROWS = np.array([3, 6, 8, 9], np.int32)
OBSTACLES = [[3.0, -0.6], [3.0, 1.4], [10.0, 20.4], [40.0, 41.5]]


def scene(gap=0.8, jitter=0.0, rate=RATE, grouped=True):
    from piml_amd.scenarios import Scenario
    extra = dict(spawn_law='clip_groups', row_unit=torch.tensor(ROW_UNIT), unit_rows=torch.tensor(UNIT_ROWS)) if grouped else \
        dict(spawn_law='clip')
    return Scenario(entries=torch.tensor(table(gap)), route_polyline=torch.zeros(0, 2), obstacles=torch.tensor(OBSTACLES),
                    time_unit=0.08, n_initial=N0, spawn_offset=jitter, arrival_radius=1.0, num_waypoints=2, spawn_cap=4,
                    arrival_rule='radius', initial_velocity=True, speed_clamp=False, fixed_spawn_rate=rate, name='clip',
                    **extra).to(DEV)


def MLAPM(**params):
    from piml_amd.models.mlapm import MLAPM as M
    return M(**params)


@functools.lru_cache(maxsize=None)
def single(seed, jitter=0.0):
    """the shared 12-frame single runs at capacity 20 (left unchanged)"""
    return MLAPM(**PLAIN).simulate_scenario(scene(jitter=jitter), T, seed=seed, capacity=CAP)


@functools.lru_cache(maxsize=None)
def ensemble(term, frames=T):
    """the shared ensembles: without the term, and with Ag = 3, group_dist = 0.25"""
    params = dict(PLAIN, Ag=AG, group_dist=GDIST) if term else PLAIN
    return MLAPM(**params).simulate_ensemble(scene(), frames, SEEDS, capacity=CAP)


def at_spawn(res):
    """what the frame wrote when each slot's agent appeared (numpy)"""
    n = res.num_agents
    m = res.mask_p[:, :n] == 1
    assert bool(m.any(0).all())
    born = m.to(torch.uint8).argmax(0)
    idx = torch.arange(n, device=born.device)
    cpu = lambda x: x.cpu().numpy()
    return dict(n=n, born=cpu(born), position=cpu(res.position[born, idx]), velocity=cpu(res.velocity[born, idx]),
                destination=cpu(res.destination[born, idx]), waypoints=cpu(res.waypoints[:, :n]),
                desired_speed=cpu(res.desired_speed[:n]), counts=cpu(res.spawn_count), spawned=res.spawned,
                dropped=res.dropped, group_first=cpu(res.group_first[:n]), group_size=cpu(res.group_size[:n]))


def replay(seed, jitter=0.0, cap=CAP, frames=T):
    return R.replay(TABLE, ROW_UNIT, UNIT_ROWS, N0, seed, frames, scene().poisson_thresholds(), cap, jitter=jitter)


def test_seeds_are_what_the_docstring_says():
    want = {4: (17, 0, 9), 11: (33, 13, 13), (1 << 63) + 4: (19, 0, 8)}
    assert sorted(want) == sorted(SEEDS)
    for seed, (spawned, dropped, n_units) in want.items():
        rp = replay(seed)
        assert (rp['spawned'], rp['dropped'], len(rp['units'])) == (spawned, dropped, n_units), seed
        if not dropped:
            assert {u for _, u, _, _ in rp['units']} == {0, 1, 2, 3}
    assert [(f, base, size) for f, _, base, size in replay(DROPPING)['units'] if base < CAP < base + size] == [(6, 18, 3)]


# ---- 1. spawns and bookkeeping ----

@pytest.mark.parametrize('jitter', [0.0, 0.25])
@pytest.mark.parametrize('seed', SEEDS)
def test_spawns_and_bookkeeping_are_the_restatements_bitwise(seed, jitter):
    res = single(seed, jitter)
    got, want = at_spawn(res), replay(seed, jitter)
    assert got['spawned'] == want['spawned'] and got['dropped'] == want['dropped'] and got['n'] == len(want['row'])
    assert (want['dropped'] > 0) == (seed == DROPPING)
    assert np.array_equal(got['counts'], want['counts']) and np.array_equal(got['born'], want['born'])
    for k in ('position', 'velocity', 'waypoints', 'desired_speed'):
        assert np.array_equal(nbits(got[k]), nbits(want[k])), k
    assert np.array_equal(nbits(got['destination']), nbits(want['waypoints'][0]))
    assert np.array_equal(got['group_first'], want['group_first']) and np.array_equal(got['group_size'], want['group_size'])
    n = got['n']                                               # slots nobody spawned into are untouched
    st = res.state
    assert (res.group_size[n:] == 0).all() and (res.group_first[n:] == 0).all()
    assert torch.isnan(st.p[n:]).all() and (st.mask[n:] == 0).all() and torch.isnan(res.position[:, n:]).all()
    assert np.array_equal(got['position'][:N0], TABLE[:N0, 0])                 # frame 0 is never jittered
    units = [(base, size, UNIT_ROWS[u]) for _, u, base, size in want['units'] if base + size <= CAP and size >= 2]
    assert len(units) >= 2
    for base, size, first in units:
        off = got['position'][base:base + size].astype(np.float64) - TABLE[first:first + size, 0]
        if jitter == 0.0:
            assert (off == 0).all()
        else:
            # one offset per unit: each member's sum rounds once, half an ulp of a coordinate below 64: 2^-19 each
            assert np.abs(off - off[0]).max() <= 2.0 ** -18 and (off != 0).all()
            assert np.abs(off).max() <= 0.25 + 2.0 ** -19
    assert res.planted_groups() == [list(range(b, min(b + s, CAP))) for b, s in
                                    [(0, 2)] + [(base, size) for _, _, base, size in want['units'] if size >= 2 and base < CAP]]


def test_a_unit_that_straddles_the_capacity_is_partly_dropped():
    res = single(DROPPING)
    assert res.spawned == 33 and res.dropped == 13 and res.num_agents == CAP
    assert res.group_first[18:].tolist() == [18, 18] and res.group_size[18:].tolist() == [3, 3]
    assert res.planted_groups()[-1] == [18, 19]
    # a larger capacity gives the same arrivals, now complete: the small run is its head
    big = MLAPM(**PLAIN).simulate_scenario(scene(), T, seed=DROPPING, capacity=40)
    assert big.spawned == 33 and big.dropped == 0 and torch.equal(big.spawn_count, res.spawn_count)
    assert torch.equal(big.group_first[:CAP], res.group_first) and torch.equal(big.group_size[:CAP], res.group_size)
    assert big.group_first[18:26].tolist() == [18, 18, 18, 21, 21, 21, 24, 25]
    assert big.group_size[18:26].tolist() == [3, 3, 3, 3, 3, 3, 1, 1] and (big.group_size[33:] == 0).all()


# ---- 2. the operator ----

def operator_rows():
    """(position, group_first, group_size): n = 1 behind a range clamped at 0; an absent mate; d == thr exactly and one ulp
    above; d = 0; a unit of 4; a unit clamped by the row count"""
    p = np.array([[1.0, 1.0],                                               # 0: first -1, size 2 -> {0}: n = 1
                  [2.0, 3.0], [NAN, NAN],                                   # 1, 2: the mate is absent
                  [0.0, 10.0], [1.0, 10.0],                                 # 3, 4: 0.5 from the centroid: d == thr at dist 0.5
                  [0.0, 12.0], [np.nextafter(np.float32(1), np.float32(2)), 12.0],   # 5, 6: 0.5 + 2^-24: just above
                  [4.0, 4.0], [4.0, 4.0],                                   # 7, 8: on top of each other: d = 0
                  [0.0, 0.0], [3.1, 0.2], [-0.4, 4.7], [2.2, 2.9],          # 9 .. 12: four
                  [7.0, 7.0], [9.5, 6.0]], np.float32)                      # 13, 14: first 13, size 4 of 15 rows
    first = np.array([-1, 1, 1, 3, 3, 5, 5, 7, 7, 9, 9, 9, 9, 13, 13], np.int32)
    size = np.array([2, 2, 2, 2, 2, 2, 2, 2, 2, 4, 4, 4, 4, 4, 4], np.int32)
    return p, first, size


@pytest.mark.parametrize('A,dist', [(3.0, 0.5), (3.0, 0.0), (0.0, 0.5), (7.25, 1.0)])
def test_group_force_is_the_restatement_bitwise(A, dist):
    from piml_amd import ops_scenario
    p, first, size = operator_rows()
    got = ops_scenario.group_force(torch.tensor(p, device=DEV), torch.tensor(first), torch.tensor(size), A, dist).cpu().numpy()
    want = R.group_force(p, first, size, A, dist)
    assert np.array_equal(nbits(got), nbits(want))
    assert (got[[0, 1, 2, 7, 8]] == 0).all()                   # n = 1, an absent mate, an absent agent, d = 0
    if (A, dist) == (3.0, 0.5):
        assert (got[[3, 4]] == 0).all() and abs(got[5, 0] - 3.0) < 1e-5 and abs(got[6, 0] + 3.0) < 1e-5 and (got[[5, 6], 1] == 0).all()
        # four: centroid (1.225, 1.95), thr 1.5: three members 2.3 .. 3.2 m away, the fourth 1.36 m, inside
        assert (np.abs(np.linalg.norm(got[9:12], axis=1) - 3.0) < 1e-5).all() and (got[12] == 0).all()
        assert (np.abs(np.linalg.norm(got[13:], axis=1) - 3.0) < 1e-5).all() and np.allclose(got[13], -got[14], rtol=1e-6)
    if (A, dist) == (3.0, 0.0):
        assert got[3, 0] == 3.0 and got[4, 0] == -3.0
    # blocks of rows: each (N, 2) block on its own, its ranges clamped to the block
    both = np.stack((p, p[::-1].copy()))
    fs = np.stack((first, first))
    got2 = ops_scenario.group_force(torch.tensor(both, device=DEV), torch.tensor(fs, device=DEV), torch.tensor(size, device=DEV),
                                    A, dist).cpu().numpy()
    assert np.array_equal(nbits(got2[0]), nbits(want))
    assert np.array_equal(nbits(got2[1]), nbits(R.group_force(both[1], first, size, A, dist)))


# ---- 3. the frame adds the operator's force ----

def test_first_frame_adds_the_operators_group_force():
    """acceleration[1] == acceleration_noterm[1] + group_force(position[0]) for the present slots, bitwise: the same
    function on the same inputs and one float32 add (the build never contracts)"""
    from piml_amd import ops_scenario
    plain, term = ensemble(False), ensemble(True)
    assert torch.equal(bits(term.position[:, 0]), bits(plain.position[:, 0]))
    G = ops_scenario.group_force(plain.position[:, 0], plain.group_first, plain.group_size, AG, GDIST)
    present = (plain.mask_p[:, 0] == 1) & (plain.mask_p[:, 1] == 1) & (term.mask_p[:, 1] == 1)
    assert present[:, :N0].all() and not present[:, N0:].any()
    want = plain.acceleration[:, 1] + G
    assert torch.equal(bits(term.acceleration[:, 1][present]), bits(want[present]))
    # the pair pulls together along y, 0.4 m from its centroid; the single feels nothing
    assert ((G[:, 0, 1] - AG).abs() < 1e-5).all() and ((G[:, 1, 1] + AG).abs() < 1e-5).all()
    assert (G[:, :2, 0] == 0).all() and (G[:, 2:] == 0).all()
    assert not torch.equal(bits(term.acceleration[:, 1, :2]), bits(plain.acceleration[:, 1, :2]))
    dt = float(plain.time_unit)
    v1 = term.velocity[:, 0] + term.acceleration[:, 1] * dt
    assert torch.equal(bits(term.velocity[:, 1][present]), bits(v1[present]))
    assert torch.equal(bits(term.position[:, 1][present]), bits((term.position[:, 0] + v1 * dt)[present]))


def test_later_frames_add_the_force_of_their_own_records():
    """every frame t: a[t + 1] of the run with the term is one MLAPM step on ITS records of frame t plus the operator's
    force on those records (arrival units included, absent mates NaN)"""
    from piml_amd import ops_scenario
    res = MLAPM(**PLAIN, Ag=AG, group_dist=GDIST).simulate_scenario(scene(), T, seed=SEEDS[0], capacity=CAP)
    dt, checked, felt = float(res.time_unit), 0, 0
    for t in range(T - 1):
        keep = (res.mask_p[t] == 1) & (res.mask_p[t + 1] == 1)
        _, frc = _step_fwd(res.position[t], res.velocity[t], res.desired_speed, res.destination[t], 'GC', dt)
        G = ops_scenario.group_force(res.position[t], res.group_first, res.group_size, AG, GDIST)
        assert torch.equal(bits(res.acceleration[t + 1][keep]), bits((frc + G)[keep])), t
        checked += int(keep.sum())
        felt += int((G[keep] != 0).any(-1).sum())
    assert checked > 60 and felt >= 8


# ---- 4. without the term ----

def test_zero_strength_is_the_run_without_the_term():
    plain = ensemble(False)
    zero = MLAPM(**PLAIN, Ag=0.0).simulate_ensemble(scene(), T, SEEDS, capacity=CAP)
    far = MLAPM(**PLAIN, Ag=AG, group_dist=50.0).simulate_ensemble(scene(), T, SEEDS, capacity=CAP)   # nobody is 50 m away
    for other in (zero, far):
        assert all(_same(other.member(m), plain.member(m)) for m in range(len(SEEDS)))
        assert all(torch.equal(getattr(other, k), getattr(plain, k)) for k in GROUP_FIELDS)


def test_without_the_term_every_frame_is_one_mlapm_step():
    frames = 40
    res = MLAPM(**PLAIN).simulate_scenario(scene(), frames, seed=SEEDS[0], capacity=64)
    assert res.dropped == 0 and res.num_agents > 30
    dt, checked = float(res.time_unit), 0
    p, v, a, d, m = res.position, res.velocity, res.acceleration, res.destination, res.mask_p
    for t in range(frames - 1):
        keep = (m[t] == 1) & (m[t + 1] == 1)
        act, frc = _step_fwd(p[t], v[t], res.desired_speed, d[t], 'GC', dt)
        assert torch.equal(bits(v[t + 1][keep]), bits(act[keep])) and torch.equal(bits(a[t + 1][keep]), bits(frc[keep])), t
        assert torch.equal(bits(p[t + 1][keep]), bits((p[t] + act * dt)[keep])), t
        checked += int(keep.sum())
    assert checked > 500


# ---- 5. members, forms, captured replays, sweeps ----

def run_state(law, walls, groups, frames=T, use_graph=False, sc=None):
    from piml_amd import scenarios
    from piml_amd.models.mlapm import MLAPM as M
    st = scenarios.scenario_state_for(sc or scene(), frames, CAP, DEV, seeds=SEEDS)
    M._run_scenario(st, law, use_graph, 4, walls=walls, groups=groups)
    return scenarios.scenario_result(st)


def same_run(a, b):
    return all(_same(a.member(m), b.member(m)) for m in range(len(SEEDS))) and \
        all(torch.equal(getattr(a, k), getattr(b, k)) for k in GROUP_FIELDS)


def same_arrivals(a, b):
    return a.spawned == b.spawned and a.dropped == b.dropped and \
        all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in ('spawn_count', 'desired_speed', 'waypoints') + GROUP_FIELDS)


def test_members_forms_and_captured_replay_are_bitwise_equal():
    from piml_amd import hip_graphs_safe, ops_scenario
    assert hip_graphs_safe()
    ens = ensemble(True)
    term = dict(PLAIN, Ag=AG, group_dist=GDIST)
    for m, s in enumerate(SEEDS):                              # member m of an ensemble is the single run
        one = MLAPM(**term).simulate_scenario(scene(), T, seed=s, capacity=CAP)
        assert _same(ens.member(m), one), m
        assert all(torch.equal(getattr(ens, k)[m], getattr(one, k)) for k in GROUP_FIELDS)
        assert ens.planted_groups(m) == one.planted_groups()
    S = len(SEEDS)
    law, glaw, wall = ops_scenario.mlapm_law(**PLAIN), ops_scenario.group_law(AG, GDIST), ops_scenario.wall_law(AW, BW)
    ltab, gtab = ops_scenario.mlapm_law_table([law] * S, DEV), ops_scenario.group_law_table([(AG, GDIST)] * S, DEV)
    wtab = ops_scenario.wall_law_table([(AW, BW)] * S, DEV)
    grid = ops_scenario.wall_grid(scene().obstacles, CUTOFF, DEV)
    base = run_state(law, None, glaw)
    assert same_run(base, ens)                                 # the by-value form is what MLAPM runs
    walled = run_state(law, (grid, wall), glaw)
    assert not torch.equal(bits(walled.position), bits(base.position)) and same_arrivals(walled, base)
    for lw in (law, ltab):
        for gl in (glaw, gtab):
            assert same_run(run_state(lw, None, gl), base)
            for wl in (wall, wtab):
                assert same_run(run_state(lw, (grid, wl), gl), walled)
    noterm = run_state(ltab, None, None)                       # no group term: the shared run without one, same arrivals
    assert same_run(noterm, ensemble(False)) and same_arrivals(noterm, base)
    assert same_arrivals(run_state(law, (grid, wtab), None), base)
    # captured: 1 eager frame + 2 replays of 4 + 2 eager
    assert same_run(run_state(ltab, (grid, wtab), gtab, use_graph=True), walled)
    assert same_run(run_state(law, None, glaw, use_graph=True), base)
    graph = MLAPM(**term).simulate_ensemble(scene(), T, SEEDS, capacity=CAP, use_graph=True)
    eager = MLAPM(**term).simulate_ensemble(scene(), T, SEEDS, capacity=CAP, use_graph=False)
    assert same_run(graph, eager) and same_run(graph, ens)
    # a one-candidate sweep is the ensemble, with and without walls
    assert same_run(MLAPM(**PLAIN).simulate_sweep(scene(), T, [term], SEEDS, capacity=CAP), ens)
    both = dict(term, Aw=AW, Bw=BW)
    assert same_run(MLAPM(**PLAIN).simulate_sweep(scene(), T, [both], SEEDS, capacity=CAP), walled)
    assert same_run(MLAPM(**both).simulate_ensemble(scene(), T, SEEDS, capacity=CAP), walled)
    # the arrivals do not depend on the law: the plain clip law's count stream is the unit count stream
    clip = MLAPM(**PLAIN).simulate_ensemble(scene(grouped=False), T, SEEDS, capacity=CAP)
    units = torch.tensor(np.stack([replay(s)['unit_counts'] for s in SEEDS]), device=DEV)
    assert torch.equal(clip.spawn_count[:, 1:].long(), units[:, 1:])


def test_sweep_run_twice_with_other_group_rows_equals_fresh_runs():
    from piml_amd.models.mlapm import SweepRun
    seeds = SEEDS[:2]
    term = dict(PLAIN, Ag=AG, group_dist=GDIST)
    first = [dict(term), dict(term, Ag=1.0, group_dist=0.5)]
    second = [dict(term, Ag=6.0, group_dist=0.0, tau=0.6), dict(term, Ag=0.0)]
    run = SweepRun(scene(), T, 2, seeds, capacity=CAP, use_graph=True, frames_per_graph=4)
    got = []
    for params in (first, second, first):
        sw = run.run(params)
        got.append(({k: getattr(sw, k).clone() for k in FIELDS + GROUP_FIELDS}, list(sw.spawned), list(sw.dropped)))
    assert run.graph is not None and run.group_table.shape == (4, 2) and run.wall_table is None
    for params, (fields, spawned, dropped) in zip((first, second, first), got):
        fresh = MLAPM(**PLAIN).simulate_sweep(scene(), T, params, seeds, capacity=CAP)
        for k in FIELDS + GROUP_FIELDS:
            assert torch.equal(bits(fields[k]), bits(getattr(fresh, k))), k
        assert spawned == fresh.spawned and dropped == fresh.dropped
        for c, p in enumerate(params):                         # and each candidate is its own ensemble
            ens = MLAPM(**p).simulate_ensemble(scene(), T, seeds, capacity=CAP)
            assert all(_same(fresh.member(c * 2 + k), ens.member(k)) for k in range(2)), c
            assert fresh.candidate(c).planted_groups(1) == ens.planted_groups(1)
    assert not torch.equal(bits(got[0][0]['position']), bits(got[1][0]['position']))
    assert torch.equal(got[0][0]['group_first'], got[1][0]['group_first'])
    with pytest.raises(ValueError):
        run.run([dict(PLAIN), dict(PLAIN)])                    # the captured frames carry the group table
    with pytest.raises(ValueError):
        MLAPM(**PLAIN).simulate_sweep(scene(), 5, [dict(term), dict(PLAIN)], seeds)


# ---- 6. behaviour ----

def test_planted_groups_are_found_by_the_group_statistics():
    """A = 0: nobody repels anybody, every agent walks straight to a waypoint hundreds of metres off, the members of a unit
    side by side 0.8 m apart at one speed -- so every planted unit present long enough is linked by the group statistics
    (closer than 2 m, the same velocity, for at least min_frames frames), deterministically"""
    frames = 60
    ens = MLAPM(**NO_PAIRS, Ag=0.0).simulate_ensemble(scene(), frames, SEEDS)
    assert ens.dropped == [0] * len(SEEDS)
    gs = ens.group_stats()
    need = gs.options['min_frames'] + 1
    found = 0
    for m in range(len(SEEDS)):
        groups = [set(g) for g in gs.groups(m)]
        for unit in ens.planted_groups(m):
            together = int((ens.mask_p[m][:, unit] == 1).all(1).sum())
            if together >= need:
                assert any(set(unit) <= g for g in groups), (m, unit)
                found += 1
        assert set(ens.planted_groups(m)[0]) == {0, 1} and any({0, 1} <= g for g in groups)
    print(f'\n[groups] {found} planted units of {sum(len(ens.planted_groups(m)) for m in range(len(SEEDS)))} present for '
          f'{need} frames or more, all found; group fraction {gs.group_fraction():.3f}')
    assert found >= len(SEEDS) and gs.group_fraction() > 0


def test_the_term_pulls_a_pair_together():
    """direction only: a pair planted 3 m apart is closer after 40 frames with Ag = 3 than with Ag = 0 (where it stays 3 m)"""
    sc = scene(gap=3.0)
    dist = {}
    for Ag in (0.0, 3.0):
        res = MLAPM(**NO_PAIRS, Ag=Ag).simulate_scenario(sc, 41, seed=SEEDS[0])
        assert (res.mask_p[40, :2] == 1).all() and res.planted_groups()[0] == [0, 1]
        dist[Ag] = float((res.position[40, 0] - res.position[40, 1]).norm())
    print(f'\n[groups] a pair planted 3 m apart, after 40 frames: {dist[0.0]:.3f} m with Ag = 0, {dist[3.0]:.3f} m with Ag = 3')
    assert dist[3.0] < dist[0.0] and abs(dist[0.0] - 3.0) < 1e-3


# ---- 7. the recorded clip ----

def test_the_gc_clips_groups_become_units_and_the_scene_runs():
    from piml_amd.groupstats import group_stats_of_raw
    from piml_amd.scenarios import clip_scenario
    raw = _raw(GC_CLIP)
    groups = group_stats_of_raw(raw).groups(0)
    assert len(groups) >= 2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sc = clip_scenario(raw, groups='auto')
        by_list = clip_scenario(raw, groups=groups)
    assert sc.spawn_law == 'clip_groups' and torch.equal(sc.row_unit, by_list.row_unit) and torch.equal(sc.unit_rows, by_list.unit_rows)
    assert torch.equal(sc.entries.view(torch.int32), by_list.entries.view(torch.int32))
    tab, row_unit, unit_rows, n0, tracks, _ = R.table(raw, groups)
    assert np.array_equal(sc.row_unit.numpy(), row_unit) and np.array_equal(sc.unit_rows.numpy(), unit_rows) and sc.n_initial == n0
    assert np.array_equal(nbits(np.delete(sc.entries.numpy(), 2, 1)), nbits(np.delete(tab, 2, 1)))
    row_of = {int(i): r for r, i in enumerate(tracks)}
    present = raw.mask_p.numpy() == 1
    shared = 0
    for g in groups:
        if not present[:, g].all(1).any():
            continue
        shared += 1
        rows = [row_of[i] for i in g]                          # one unit, or the consecutive cuts of one: consecutive rows
        assert rows == list(range(rows[0], rows[0] + len(g))), g
        at = 0
        while at < len(g):                                     # each cut starts a unit of min(4, what is left) members
            size = min(4, len(g) - at)
            assert [row_unit[rows[at] + q].tolist() for q in range(size)] == [[q, size] for q in range(size)], g
            at += size
    assert shared >= 2
    ens = MLAPM(**PLAIN).simulate_ensemble(sc.to(DEV), 60, [0, 1, 2])
    assert ens.dropped == [0, 0, 0] and min(ens.spawned) >= sc.n_initial
    print(f'\n[groups] GC clip: {len(groups)} groups, {shared} with a shared frame; capacity {ens.capacity}, spawned {ens.spawned}, '
          f'planted units {[len(ens.planted_groups(m)) for m in range(3)]}')


# ---- 8. the command line and the errors ----

def test_errors():
    from piml_amd import ops_scenario, scenarios, simulate
    grouped, plain = scene(), scene(grouped=False)
    st = scenarios.scenario_state_for(grouped, 4, CAP, DEV, seeds=SEEDS)
    with pytest.raises(ValueError, match='clip_groups'):
        ops_scenario.scenario_step(st, init=True)              # the network's frame has no group arrivals
    with pytest.raises(ValueError, match='clip_groups'):
        ops_scenario.scenario_step(st, torch.zeros(len(SEEDS), CAP, 2, device=DEV))
    law, glaw = ops_scenario.mlapm_law(), ops_scenario.group_law(AG, GDIST)
    ops_scenario.scenario_step_mlapm(st, None, init=True)
    with pytest.raises(ValueError):
        ops_scenario.scenario_step_mlapm(st, law, groups=ops_scenario.group_law_table([(AG, GDIST)] * 2, DEV))
    with pytest.raises(TypeError):
        ops_scenario.scenario_step_mlapm(st, law, groups=(AG, GDIST))
    assert int(st.t.item()) == 0 and int(st.spawned[0, 0]) == N0
    ops_scenario.scenario_state_reset(st)
    assert (st.group_size == 0).all() and (st.group_first == 0).all() and int(st.spawned.sum()) == 0
    pst = scenarios.scenario_state_for(plain, 4, CAP, DEV, seeds=SEEDS)
    ops_scenario.scenario_step_mlapm(pst, None, init=True)      # (a scene without groups: scenario_step's init launch)
    with pytest.raises(ValueError, match='no groups'):
        ops_scenario.scenario_step_mlapm(pst, law, groups=glaw)
    with pytest.raises(ValueError, match='no groups'):
        MLAPM(**PLAIN, Ag=AG).simulate_scenario(plain, 5)
    with pytest.raises(ValueError, match='no groups'):
        MLAPM(**PLAIN).simulate_sweep(plain, 5, [dict(PLAIN, Ag=AG)], SEEDS)
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'pinnsf', '--scene-from', 'clip.npy', '--scene-groups', 'auto'])


def test_the_command_line(tmp_path):
    from piml_amd.groupstats import ADDITIVE, GroupStats, group_stats_of_raw
    from piml_amd.scenarios import clip_scenario
    clip = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    raw = _raw(GC_CLIP)
    groups = group_stats_of_raw(raw).groups(0)
    term = dict(PLAIN, Ag=AG, group_dist=0.5)
    (tmp_path / 'groups.json').write_text(json.dumps(groups))
    (tmp_path / 'law.json').write_text(json.dumps(term))
    out = tmp_path / 'stats.json'
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--params', str(tmp_path / 'law.json'),
                        '--scene-from', clip, '--scene-groups', str(tmp_path / 'groups.json'), '--frames', '40', '--seeds', '0:2',
                        '--group-stats', str(out)], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = GroupStats.from_json(str(out))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sc = clip_scenario(raw, groups=groups).to(DEV)
    want = MLAPM(**term).simulate_ensemble(sc, 40, [0, 1]).group_stats()
    assert all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ADDITIVE)
    # Ag in the file on a scene without groups: a message, not a traceback
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--params', str(tmp_path / 'law.json'),
                        '--scene-from', clip, '--frames', '4', '--group-stats', str(out)], cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and 'no groups' in p.stderr and 'Traceback' not in p.stderr
