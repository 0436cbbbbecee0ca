"""CPU: a recorded clip's groups as arrival units (`scenarios.clip_scenario(groups=)`, spawn law 'clip_groups' =
PIML_SPAWN_CLIP_GROUPS) on a hand-made clip of 15 tracks x 60 frames: the unit rules against their restatement
(tests/scenario_groups_ref.py) and against the rows worked out by hand, groups=None and groups=[] against today's scene,
the builder's errors, the restatement's own properties, the exported symbols and the argument checks of the new entries,
which return before any launch and so run without a GPU.

The clip (D = 2; a track is present over [enter, leave)):
  0, 1    a pair present at frame 0                            -> initial unit (0, 1)
  2       a single at frame 0, grouped with 14, which never appears -> initial single
  3, 4, 5 a triple entering at frames 8, 10, 10                -> arrival unit at f_u = 10 (track 3's waypoint index moved at 9)
  6 .. 10 a group of five entering at 20, 20, 21, 22, 22       -> f_u = 22, cut into (6, 7, 8, 9) and (10)
  11, 12  a group whose members never share a frame (5..15, 30..45) -> singles at 5 and 30
  13      a single entering at 12
  14      never present"""
import ctypes
import os
import types
import warnings

import numpy as np
import pytest
import torch

import scenario_clip_ref as CR
import scenario_groups_ref as R
from conftest import REPO, bits
from test_abi import declared_symbols

INVALID = 1                                                   # hipErrorInvalidValue
T, N, D = 60, 15, 2
SPANS = [(0, 40), (0, 50), (0, 30), (8, 55), (10, 55), (10, 55), (20, 60), (20, 60), (21, 60), (22, 60), (22, 60), (5, 15),
         (30, 45), (12, 50), (0, 0)]
GROUPS = [[1, 0], [2, 14], [5, 3, 4], [6, 7, 8, 9, 10], [11, 12]]
# (tracks, f_u) in row order
INITIAL = [([0, 1], 0), ([2], 0)]
ARRIVALS = [([3, 4, 5], 10), ([6, 7, 8, 9], 22), ([10], 22), ([11], 5), ([12], 30), ([13], 12)]


def make_raw():
    pos = torch.full((T, N, 2), float('nan'))
    vel = torch.zeros(T, N, 2)
    mask = torch.zeros(T, N)
    for i, (a, b) in enumerate(SPANS):
        t = torch.arange(a, b, dtype=torch.float32)
        pos[a:b, i, 0], pos[a:b, i, 1] = 0.125 * t + i, 0.5 * i + 0.015625 * t
        vel[a:b, i, 0], vel[a:b, i, 1] = 1.0 + i / 16.0, 0.125
        mask[a:b, i] = 1
    way = torch.zeros(D, N, 2)
    way[0, :, 0], way[0, :, 1] = 20.0, torch.arange(N, dtype=torch.float32)
    way[1, :, 0], way[1, :, 1] = 40.0, torch.arange(N, dtype=torch.float32) + 0.5
    way[1, 13] = float('nan')                                 # a track with one waypoint
    didx = torch.zeros(T, N, dtype=torch.long)
    didx[9:, 3] = 1                                           # track 3 heads for its second waypoint from frame 9 on
    return types.SimpleNamespace(position=pos, velocity=vel, mask_p=mask, waypoints=way, dest_idx=didx,
                                 obstacles=torch.tensor([[1.0, 2.0], [3.0, 4.0]]), time_unit=0.08)


@pytest.fixture(scope='module')
def raw():
    return make_raw()


@pytest.fixture(scope='module')
def grouped(raw):
    from piml_amd.scenarios import clip_scenario
    with pytest.warns(UserWarning) as rec:
        sc = clip_scenario(raw, groups=GROUPS)
    return sc, [str(w.message) for w in rec]


def same_table(got, want):
    """bitwise but for point 2, the desired speed, which the restatements average in float64"""
    return got.shape == want.shape and np.array_equal(bits(np.delete(got, 2, 1)), bits(np.delete(want, 2, 1))) and \
        np.allclose(got[:, 2], want[:, 2], rtol=25 * 2.0 ** -24, atol=0)


def test_rows_units_and_rate(raw, grouped):
    from piml_amd.scenarios import CLIP_MAX_GROUP, Scenario
    sc, messages = grouped
    assert CLIP_MAX_GROUP == 4 and isinstance(sc, Scenario)
    assert sc.spawn_law == 'clip_groups' and sc.arrival_rule == 'radius' and sc.num_waypoints == D
    units = INITIAL + ARRIVALS
    tracks = [i for u, _ in units for i in u]
    frames = [f for u, f in units for _ in u]
    tab = sc.entries.numpy()
    assert tab.shape == (14, 3 + D, 2) and tab.dtype == np.float32 and sorted(tracks) == list(range(14))
    assert sc.n_initial == 3
    pos, vel = raw.position.numpy(), raw.velocity.numpy()
    assert np.array_equal(bits(tab[:, 0]), bits(pos[frames, tracks])) and np.array_equal(bits(tab[:, 1]), bits(vel[frames, tracks]))
    from piml_amd.data.data import desired_speed_per_agent
    assert np.array_equal(tab[:, 2, 0], desired_speed_per_agent(raw.velocity, 25).numpy()[tracks]) and (tab[:, 2, 1] == 0).all()
    # the waypoints ahead at f_u: track 3 (row 3) has passed its first one at frame 10, track 13 (row 13) has only one
    way = raw.waypoints.numpy()
    for r, i in enumerate(tracks):
        want = np.stack((way[1, i], [np.nan, np.nan])) if i == 3 else way[:, i]
        assert np.array_equal(bits(tab[r, 3:]), bits(want)), (r, i)
    assert np.isnan(tab[[3, 13], 4]).all() and not np.isnan(np.delete(tab, [3, 13], 0)[:, 3:]).any()
    assert sc.row_unit.dtype == torch.int32 and sc.unit_rows.dtype == torch.int32
    assert sc.row_unit.tolist() == [[q, len(u)] for u, _ in units for q in range(len(u))]
    assert sc.unit_rows.tolist() == [3, 6, 10, 11, 12, 13]
    assert sc.fixed_spawn_rate == 6 / 59 and sc.spawn_rate == 6 / 59 and sc.spawn_cap == 8
    assert sum('never share a frame' in m and m.startswith('clip_scenario: 1 ') for m in messages) == 1
    assert sum('cut into units' in m and m.startswith('clip_scenario: 1 ') for m in messages) == 1 and len(messages) == 2
    # the restatement builds the same table row by row (its float64 mean speed against torch's float32 one: 25 terms)
    want = R.table(raw, GROUPS)
    assert same_table(tab, want[0]) and np.array_equal(sc.row_unit.numpy(), want[1])
    assert np.array_equal(sc.unit_rows.numpy(), want[2]) and sc.n_initial == want[3]
    assert want[4].tolist() == tracks and want[5].tolist() == frames
    assert R.units(raw.mask_p.numpy() == 1, GROUPS)[:2] == (INITIAL, ARRIVALS)
    moved = sc.to('cpu')                                      # .to() carries the new fields
    assert torch.equal(moved.row_unit, sc.row_unit) and torch.equal(moved.unit_rows, sc.unit_rows)


def test_a_member_already_present_arrives_with_its_group(raw):
    """the window (9, 60): track 3 walks at frame 9, its group's f_u is 10 -- it is an arrival row, not in the first frame"""
    from piml_amd.scenarios import clip_scenario
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sc = clip_scenario(raw, frames=(9, 60), groups=GROUPS)
    initial, arrivals, _ = R.units(raw.mask_p.numpy() == 1, GROUPS, (9, 60))
    assert initial == [([0, 1], 9), ([2], 9), ([11], 9)] and arrivals[0] == ([3, 4, 5], 10)
    assert sc.n_initial == 4 and sc.unit_rows.tolist()[0] == 4 and sc.row_unit[4].tolist() == [0, 3]
    assert np.array_equal(sc.entries.numpy()[4, 0], raw.position.numpy()[10, 3])
    want = R.table(raw, GROUPS, (9, 60))
    assert same_table(sc.entries.numpy(), want[0]) and np.array_equal(sc.row_unit.numpy(), want[1])
    assert sc.fixed_spawn_rate == len(arrivals) / 50
    plain = clip_scenario(raw, frames=(9, 60))                # today's scene has track 3 in its first frame
    assert plain.n_initial == 5 and plain.entries.shape[0] == sc.entries.shape[0]


def test_groups_none_is_todays_scene(raw):
    from piml_amd.scenarios import clip_scenario
    for window in (None, (9, 60)):
        sc = clip_scenario(raw, frames=window)
        tab, n0, _, _ = CR.table(raw, window)
        assert sc.spawn_law == 'clip' and sc.row_unit is None and sc.unit_rows is None
        assert sc.n_initial == n0 and same_table(sc.entries.numpy(), tab)
        again = clip_scenario(raw, frames=window, groups=None)
        assert torch.equal(again.entries.view(torch.int32), sc.entries.view(torch.int32)) and vars(again).keys() == vars(sc).keys()
        for k, v in vars(sc).items():
            if not isinstance(v, torch.Tensor):
                assert getattr(again, k) == v, k
            else:
                assert torch.equal(getattr(again, k).view(torch.int32), v.view(torch.int32)), k


def test_no_groups_is_todays_table_under_the_new_law(raw):
    from piml_amd.scenarios import clip_scenario, default_capacity
    for window in (None, (9, 60)):
        plain = clip_scenario(raw, frames=window)
        sc = clip_scenario(raw, frames=window, groups=[])
        assert sc.spawn_law == 'clip_groups' and plain.spawn_law == 'clip'
        assert torch.equal(sc.entries.view(torch.int32), plain.entries.view(torch.int32))
        E = sc.entries.shape[0]
        assert sc.n_initial == plain.n_initial and sc.fixed_spawn_rate == plain.fixed_spawn_rate and sc.spawn_cap == plain.spawn_cap
        assert sc.row_unit.tolist() == [[0, 1]] * E and sc.unit_rows.tolist() == list(range(sc.n_initial, E))
        assert default_capacity(sc, 60) == default_capacity(plain, 60)


def test_default_capacity_bounds_by_the_largest_arrival_unit(grouped):
    from piml_amd.scenarios import default_capacity
    import dataclasses
    sc, _ = grouped
    singles = dataclasses.replace(sc, row_unit=None, unit_rows=None)
    q = default_capacity(singles, 60) - sc.n_initial          # the unit quantile
    assert q >= 1 and default_capacity(sc, 60) == sc.n_initial + 4 * q
    assert default_capacity(sc, 1) == sc.n_initial


@pytest.mark.parametrize('bad', [[[0, 15]], [[0, -1]], [[0, 1], [1, 2]], [[0, 0]], [[3]], [[]], 'all'])
def test_builder_errors(raw, bad):
    from piml_amd.scenarios import clip_scenario
    with pytest.raises(ValueError):
        clip_scenario(raw, groups=bad)


def test_the_unit_tail_check_counts_units(raw):
    """12 arrival tracks in a 3-frame window are 6 per frame as singles (refused at spawn_cap 8: P(K > 8 | 6) = 0.15) and 3
    units per frame in groups of 4 (P(K > 8 | 1.5) = 2.6e-5 -- still refused; in a 10-frame window, 0.33 per frame, fine)"""
    from piml_amd.scenarios import clip_scenario
    r = make_raw()
    r.mask_p[:] = 0
    r.mask_p[:, 0] = 1                                         # one track at frame 0
    r.mask_p[1:, 1:13] = 1                                     # twelve enter at frame 1
    r.position = torch.where(r.mask_p.bool().unsqueeze(-1), torch.ones_like(r.position), torch.full_like(r.position, float('nan')))
    groups = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]]
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(r, frames=(0, 3), groups=[])
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(r, frames=(0, 3), groups=groups)
    sc = clip_scenario(r, frames=(0, 10), groups=groups)
    assert sc.fixed_spawn_rate == 3 / 9 and sc.unit_rows.tolist() == [1, 5, 9] and sc.n_initial == 1
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(r, frames=(0, 10), groups=[])            # 12 / 9 singles per frame: P(K > 8) = 4e-6


# ---- the restatement's own properties ----

@pytest.fixture(scope='module')
def replays(grouped):
    sc, _ = grouped
    tab, ru, ur = sc.entries.numpy(), sc.row_unit.numpy(), sc.unit_rows.numpy()
    import dataclasses
    fast = dataclasses.replace(sc, fixed_spawn_rate=1.5)      # enough draws in a short run
    return {(seed, cap): R.replay(tab, ru, ur, sc.n_initial, seed, 120, fast.poisson_thresholds(), cap)
            for seed in (0, 3, (1 << 63) + 1) for cap in (40, 4096)}, (tab, ru, ur, sc.n_initial)


def test_every_unit_is_reachable_by_the_draw(replays):
    runs, (tab, ru, ur, n0) = replays
    drawn = {u for (seed, cap), rp in runs.items() if cap == 4096 for _, u, _, _ in rp['units']}
    assert drawn == set(range(len(ur)))
    # the integer map reaches both ends: word 0 -> unit 0, word 2^32 - 1 -> the last unit
    Ua = len(ur)
    assert ((0 >> 8) * Ua) >> 24 == 0 and (((0xffffffff >> 8) * Ua) >> 24) == Ua - 1


def test_slots_of_a_unit_are_consecutive_and_the_counts_add_up(replays):
    runs, (tab, ru, ur, n0) = replays
    for (seed, cap), rp in runs.items():
        n = len(rp['row'])
        assert rp['spawned'] == n0 + sum(s for _, _, _, s in rp['units']) == int(rp['counts'].sum())
        assert rp['dropped'] == max(0, rp['spawned'] - cap) and n == min(rp['spawned'], cap)
        assert (rp['dropped'] > 0) == (cap == 40)
        assert rp['unit_counts'].sum() == len(rp['units']) and (rp['counts'][1:] >= rp['unit_counts'][1:]).all()
        nxt = n0
        for f, u, base, size in rp['units']:                   # units tile the slots in order
            assert base == nxt and size == ru[ur[u], 1]
            nxt += size
            for q in range(size):
                if base + q < cap:
                    s = base + q
                    assert rp['row'][s] == ur[u] + q and rp['born'][s] == f
                    assert rp['group_first'][s] == base and rp['group_size'][s] == size
        first, size = rp['group_first'], rp['group_size']
        assert ((np.arange(n) >= first) & (np.arange(n) < first + size)).all()
        assert first[:n0].tolist() == [0, 0, 2] and size[:n0].tolist() == [2, 2, 1]
    # the arrivals do not depend on the capacity: the small run is the large one's head
    for seed in (0, 3, (1 << 63) + 1):
        small, large = runs[(seed, 40)], runs[(seed, 4096)]
        assert small['units'] == large['units'] and np.array_equal(small['row'], large['row'][:40])


def test_group_force_restatement_by_hand():
    p = np.array([[0, 0], [3, 0], [np.nan, np.nan], [0, 4], [1, 1]], np.float32)
    first, size = np.array([0, 0, 0, 0, 4], np.int32), np.array([4, 4, 4, 4, 1], np.int32)
    G = R.group_force(p, first, size, 2.0, 0.5)
    # three present mates: c = (1, 4/3), thr = 1; row 0: e = c, |e| = 5/3 > 1
    c = np.array([np.float32(1.0), np.float32(4.0) / np.float32(3.0)], np.float32)
    d = np.sqrt(np.float32(c[0] * c[0]) + np.float32(c[1] * c[1]), dtype=np.float32)
    assert np.array_equal(G[0], (np.float32(2.0) * c / d).astype(np.float32))
    assert (G[2] == 0).all() and (G[4] == 0).all() and G[1, 0] < 0 < G[1, 1] and G[3, 1] < 0 < G[3, 0]
    assert np.allclose(np.linalg.norm(G[[0, 1, 3]], axis=1), 2.0, rtol=1e-6)
    assert (R.group_force(p, first, size, 2.0, 3.0) == 0).all()              # everyone within dist (n - 1) = 6 m


# ---- the library: symbols and argument checks (no launch, no GPU) ----

def test_symbols_and_ids():
    from piml_amd import _lib
    names = {'piml_group_force', 'piml_scenario_step_mlapm_groups'}
    assert names <= set(declared_symbols(('piml_hip.h',))) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.piml_abi_version() == 35 == _lib.ABI_VERSION
    assert _lib.SPAWN_CLIP_GROUPS == 7 and 7 not in _lib.SPAWN_LAWS.values()
    header = open(os.path.join(REPO, 'include', 'piml_hip.h')).read()
    assert 'PIML_SPAWN_CLIP_GROUPS = 7' in header
    assert ctypes.sizeof(_lib.GroupLaw) == 8 and ctypes.sizeof(_lib.SceneGroups) == 40


def _descriptor(law=7):
    """a grouped clip descriptor that passes every check, over pointers nobody dereferences: 5 rows, 2 initial, D = 2"""
    from piml_amd import _lib
    s = _lib.Scenario()
    for name, _ in _lib.Scenario._fields_[:23]:
        setattr(s, name, 0x1000)
    s.hist_width, s.F, s.D, s.E, s.P, s.R = 2, 7, 2, 5, 5, 0
    s.capacity, s.T, s.n_initial, s.route_max_iters, s.spawn_cap = 16, 12, 2, 0, 4
    s.dt, s.arrival_radius = 0.08, 1.0
    for j, x in enumerate((1000, 5000, 9000, 12000)):
        s.poisson_thresholds[j] = x
    r = _lib.ScenarioRules()
    r.spawn_law, r.arrival_rule, r.initial_velocity = law, _lib.ARRIVAL_RULES['radius'], 1
    g = _lib.SceneGroups()
    g.row_unit = g.unit_rows = g.group_first = g.group_size = 0x1000
    g.n_units = 2
    return s, r, g


def test_entry_checks_return_before_any_launch():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    law = ops_scenario.mlapm_law()
    glaw = ops_scenario.group_law(3.0, 0.5)
    wall = ops_scenario.wall_law(50.0, -5.0)

    def call(s, r, g, members=2, sd=seeds, law=law, table=None, grid=None, wall=None, wtable=None, glaw=None, gtable=None,
             init=0, offset=0):
        ref = lambda x: None if x is None else (x if isinstance(x, int) else ctypes.byref(x))
        return L.piml_scenario_step_mlapm_groups(ref(s), ref(r), members, sd, ref(law), table, ref(grid), ref(wall), wtable,
                                                 ref(g), ref(glaw), gtable, init, offset, None)
    s, r, g = _descriptor()
    assert call(None, r, g) == call(s, None, g) == call(s, r, None) == call(s, r, g, sd=None) == INVALID
    assert call(s, r, g, members=0) == call(s, r, g, members=65536) == call(s, r, g, offset=-1) == INVALID
    assert call(s, r, g, init=2) == call(s, r, g, init=-1) == INVALID
    for law_id in range(7):                                   # only PIML_SPAWN_CLIP_GROUPS comes here
        assert call(s, _descriptor(law_id)[1], g) == INVALID and call(s, _descriptor(law_id)[1], g, init=1) == INVALID
    for field, value in (('P', 4), ('capacity', 0), ('entries', None), ('n_initial', 6), ('n_initial', 5), ('spawn_cap', 9),
                         ('position_out', None), ('D', 9)):   # the existing frame checks, init launch included
        s2 = _descriptor()[0]
        setattr(s2, field, value)
        assert call(s2, r, g) == INVALID and call(s2, r, g, init=1) == INVALID, field
    for field in ('row_unit', 'unit_rows', 'group_first', 'group_size'):
        g2 = _descriptor()[2]
        setattr(g2, field, None)
        assert call(s, r, g2) == INVALID and call(s, r, g2, init=1) == INVALID, field
    for n_units in (-1, 0, (1 << 24) + 1):
        g2 = _descriptor()[2]
        g2.n_units = n_units
        assert call(s, r, g2) == INVALID and call(s, r, g2, init=1) == INVALID, n_units
    for A, dist in ((float('nan'), 0.5), (float('inf'), 0.5), (-1.0, 0.5), (3.0, float('nan')), (3.0, float('inf')), (3.0, -0.5)):
        bad = _lib.GroupLaw()
        bad.A, bad.dist = A, dist
        assert call(s, r, g, glaw=bad) == INVALID and call(s, r, g, glaw=bad, init=1) == INVALID, (A, dist)
    assert call(s, r, g, glaw=glaw, gtable=0x1000) == INVALID and call(s, r, g, glaw=glaw, gtable=0x1000, init=1) == INVALID
    # the law and wall forms of a frame
    assert call(s, r, g, law=None) == call(s, r, g, table=0x1000) == INVALID
    bad_law = ops_scenario.mlapm_law()
    bad_law.tau = 0.0
    assert call(s, r, g, law=bad_law) == INVALID
    assert call(s, r, g, wall=wall) == call(s, r, g, wtable=0x1000) == INVALID        # a wall law without a grid
    grid = _lib.WallGrid()                                    # (an all-zero grid fails the grid checks)
    assert call(s, r, g, grid=grid, wall=wall) == INVALID
    ok = ops_scenario.wall_grid_desc(ops_scenario.wall_grid_host(np.array([[0.0, 0.0], [1.0, 1.0]], np.float32)), 0x1000, 0x1000)
    assert call(s, r, g, grid=ok) == call(s, r, g, grid=ok, wall=wall, wtable=0x1000) == INVALID
    # piml_group_force
    assert L.piml_group_force(0x1000, 0x1000, 0x1000, -1, 3.0, 0.5, 0x1000, None) == INVALID
    for A, dist in ((float('nan'), 0.5), (-1.0, 0.5), (3.0, -0.5), (3.0, float('inf'))):
        assert L.piml_group_force(0x1000, 0x1000, 0x1000, 4, A, dist, 0x1000, None) == INVALID
    for k in range(4):
        ptrs = [0x1000] * 4
        ptrs[k] = None
        assert L.piml_group_force(ptrs[0], ptrs[1], ptrs[2], 4, 3.0, 0.5, ptrs[3], None) == INVALID
    assert L.piml_group_force(None, None, None, 0, 3.0, 0.5, None, None) == 0                # nothing to do, nothing launched


def test_existing_entries_still_reject_the_grouped_law():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    s, r, _ = _descriptor()
    d, rr = ctypes.byref(s), ctypes.byref(r)
    law, wall = ops_scenario.mlapm_law(), ops_scenario.wall_law(50.0, -5.0)
    ok = ops_scenario.wall_grid_desc(ops_scenario.wall_grid_host(np.array([[0.0, 0.0], [1.0, 1.0]], np.float32)), 0x1000, 0x1000)
    assert L.piml_scenario_step_rules(d, rr, None, 1, None) == INVALID
    assert L.piml_scenario_step_rules(d, rr, 0x1000, 0, None) == INVALID
    assert L.piml_scenario_step_members(d, rr, 2, seeds, None, 1, None) == INVALID
    assert L.piml_scenario_step_members(d, rr, 2, seeds, 0x1000, 0, None) == INVALID
    assert L.piml_scenario_step_mlapm(d, rr, 2, seeds, ctypes.byref(law), 0, None) == INVALID
    assert L.piml_scenario_step_mlapm_laws(d, rr, 2, seeds, 0x1000, 0, None) == INVALID
    assert L.piml_scenario_step_mlapm_walls(d, rr, 2, seeds, ctypes.byref(law), None, ctypes.byref(ok), ctypes.byref(wall), None,
                                            0, None) == INVALID


# ---- Python plumbing that needs no GPU ----

BASE = {'version': 'GC', 'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}


def test_mlapm_accepts_the_group_constants(grouped):
    from piml_amd import ops_scenario, scenarios
    from piml_amd.models import mlapm
    assert mlapm.group_args(BASE) is None
    assert mlapm.group_args({**BASE, 'Ag': 3}) == (3.0, 0.5) and mlapm.group_args({**BASE, 'Ag': 0, 'group_dist': 0.25}) == (0.0, 0.25)
    mlapm.MLAPM(**BASE, Ag=3.0, group_dist=1.0)
    for bad in (dict(group_dist=0.5), dict(Ag=-1.0), dict(Ag=float('nan')), dict(Ag=3.0, group_dist=-0.5),
                dict(Ag=3.0, group_dist=float('inf'))):
        with pytest.raises(ValueError):
            mlapm.MLAPM(**BASE, **bad)
    for bad in ((-1.0, 0.5), (float('inf'), 0.5), (3.0, -1.0)):
        with pytest.raises(ValueError):
            ops_scenario.group_law(*bad)
    g = ops_scenario.group_law(3, 0.5)
    assert (g.A, g.dist) == (3.0, 0.5)
    # Ag needs a scene with groups: refused before any state is allocated
    sim = mlapm.MLAPM(**BASE, Ag=3.0)
    for sc in (scenarios.crosswalk_scenario(), scenarios.gc_scenario()):
        with pytest.raises(ValueError, match='no groups'):
            sim.simulate_scenario(sc, 5, device='cpu')
        with pytest.raises(ValueError, match='no groups'):
            sim.simulate_ensemble(sc, 5, [0, 1], device='cpu')
        with pytest.raises(ValueError, match='no groups'):
            sim.simulate_sweep(sc, 5, [{**BASE, 'Ag': 3.0}], [0], device='cpu')
    mlapm.check_scene_groups(grouped[0])
    # sweeps: every candidate or none
    with_g = {**BASE, 'Ag': 3.0}
    assert len(mlapm.sweep_laws([with_g, {**with_g, 'Ag': 1.0, 'group_dist': 0.25}])) == 2
    assert mlapm.sweep_groups([with_g, {**with_g, 'Ag': 1.0, 'group_dist': 0.25}]) == [(3.0, 0.5), (1.0, 0.25)]
    assert mlapm.sweep_groups([BASE, BASE]) is None
    for mixed in ([with_g, BASE], [{**BASE, 'group_dist': 0.5}], [{**with_g, 'Ag': -3.0}]):
        with pytest.raises(ValueError):
            mlapm.sweep_laws(mixed)


def test_command_line_flags(tmp_path):
    import json
    from piml_amd.simulate import get_args, load_mlapm_params
    good = tmp_path / 'groups.json'
    good.write_text(json.dumps([[0, 1], [3, 4, 5]]))
    own, _ = get_args(['--law', 'mlapm', '--scene-from', 'clip.npy', '--scene-groups', str(good)])
    assert own.scene_groups == [[0, 1], [3, 4, 5]]
    own, _ = get_args(['--law', 'mlapm', '--scene-from', 'clip.npy', '--scene-groups', 'auto'])
    assert own.scene_groups == 'auto'
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps({'groups': [[0, 1]]}))
    for argv in (['--scene-from', 'clip.npy', '--scene-groups', 'auto'],                       # the network's frame
                 ['--law', 'pinnsf', '--scene-from', 'clip.npy', '--scene-groups', str(good)],
                 ['--law', 'mlapm', '--scene-groups', 'auto'],                                # no --scene-from
                 ['--law', 'mlapm', '--scene-from', 'clip.npy', '--scene-groups', str(bad)],
                 ['--law', 'mlapm', '--scene-from', 'clip.npy', '--scene-groups', str(tmp_path / 'missing.json')]):
        with pytest.raises(SystemExit) as ex:
            get_args(argv)
        assert ex.value.code != 0, argv
    params = tmp_path / 'p.json'
    params.write_text(json.dumps({'Ag': 3.0, 'group_dist': 0.75, 'tau': 0.6}))
    got = load_mlapm_params(str(params))
    assert got['Ag'] == 3.0 and got['group_dist'] == 0.75 and got['tau'] == 0.6 and got['version'] == 'GC'
    for text in ({'group_dist': 0.5}, {'Ag': -1.0}, {'Ag': 'three'}):
        params.write_text(json.dumps(text))
        with pytest.raises(ValueError):
            load_mlapm_params(str(params))


def test_results_carry_the_planted_groups():
    from piml_amd.scenarios import ScenarioEnsemble, ScenarioResult
    z = torch.zeros(3, 6, 2)
    res = ScenarioResult(position=z, spawned=7, group_first=torch.tensor([0, 0, 2, 3, 3, 3]), group_size=torch.tensor([2, 2, 1, 4, 4, 4]))
    assert res.planted_groups() == [[0, 1], [3, 4, 5]]        # the unit of four was cut by the capacity
    assert ScenarioResult(position=z, spawned=2).planted_groups() == []
    assert ScenarioResult(position=z, spawned=2, group_first=torch.zeros(6, dtype=torch.int32),
                          group_size=torch.tensor([2, 2, 0, 0, 0, 0])).planted_groups() == [[0, 1]]
    field = lambda *shape: torch.zeros(2, *shape)
    ens = ScenarioEnsemble(position=field(3, 6, 2), velocity=field(3, 6, 2), acceleration=field(3, 6, 2), destination=field(3, 6, 2),
                           mask_p=field(3, 6), waypoints=field(1, 6, 2), desired_speed=field(6), spawn_count=field(3),
                           obstacles=None, time_unit=0.08, capacity=6, seeds=[0, 1], spawned=[6, 3], dropped=[0, 0],
                           group_first=torch.tensor([[0, 0, 2, 3, 3, 3], [0, 1, 1, 0, 0, 0]]),
                           group_size=torch.tensor([[2, 2, 1, 3, 3, 3], [1, 2, 2, 0, 0, 0]]))
    assert ens.planted_groups() == [[0, 1], [3, 4, 5]] and ens.planted_groups(1) == [[1, 2]]
    assert ens.member(1).group_size.tolist() == [1, 2, 2, 0, 0, 0]
    del ens.group_first, ens.group_size                       # an ensemble of a scene without groups
    assert ens.member(0).group_first is None and ens.planted_groups() == []
