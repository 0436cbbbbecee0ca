"""CPU: the reference's synthetic scenes (crosswalk, four_directional_square, basic_unit1..3, src/data/scenarios.py:9-311)
as piml_amd.scenarios factories -- their deterministic geometry against the reference (tests/golden/scenario_synth.npz,
tests/golden/make_scenario_synth.py), the numpy restatement of their spawn laws (tests/scenario_synth_ref.py) on the
reference's supports, and the argument checks of piml_scenario_step_rules (no launch)."""
import ctypes

import numpy as np
import pytest
import torch

import scenario_synth_ref as R
from conftest import golden

SYNTH = ('crosswalk', 'four_directional_square', 'basic_unit1', 'basic_unit2', 'basic_unit3')


def factory(name, **kw):
    from piml_amd.scenarios import SCENARIOS
    return SCENARIOS[name](**kw)


def test_every_scenario_builds():
    from piml_amd.scenarios import SCENARIOS, default_capacity
    assert set(SYNTH) | {'gc'} == set(SCENARIOS)
    for name, make in SCENARIOS.items():
        sc = make(time_unit=0.08, uniform_desired_speed=False)
        assert sc.name == name and sc.obstacles.shape[-1] == 2 and sc.n_initial >= 1
        assert sc.num_waypoints == (2 if name in ('gc', 'crosswalk') else 1)
        assert default_capacity(sc, 300) >= sc.n_initial
    assert factory('four_directional_square').uniform_desired_speed and factory('basic_unit2').uniform_desired_speed
    assert not factory('crosswalk').uniform_desired_speed


def test_square_geometry_is_the_references_bit_for_bit():
    from piml_amd.scenarios import square_layout
    g = golden('scenario_synth')
    sc = factory('four_directional_square')
    pos, dst = square_layout(sc)
    assert np.array_equal(pos.numpy(), g['four_directional_square/unshuffled/position'])
    assert np.array_equal(dst.numpy(), g['four_directional_square/unshuffled/waypoints'][0])
    assert np.array_equal(pos.numpy(), g['four_directional_square/frame0/position'])     # randperm moves destinations only
    assert np.array_equal(sc.obstacles.numpy(), g['four_directional_square/frame0/obstacles'])
    assert sc.n_initial == 100 and sc.spawn_cap == 0 and default_capacity_of(sc) == 100
    # the reference's frame-0 destinations are the unshuffled ones under one permutation shared by the four blocks
    ref = g['four_directional_square/frame0/waypoints'][0].reshape(4, 25, 2)
    un = dst.numpy().reshape(4, 25, 2)
    perm = [int(np.nonzero((un[0] == ref[0, c]).all(1))[0][0]) for c in range(25)]
    assert sorted(perm) == list(range(25)) and all(np.array_equal(un[b][perm], ref[b]) for b in range(4))
    # and the restatement's permutation is one
    assert sorted(R.square_perm(3, 5).tolist()) == list(range(25))


def default_capacity_of(sc):
    from piml_amd.scenarios import default_capacity
    return default_capacity(sc, 500)


def ref_cols(key):
    """the reference's generated columns of `key` (tests/golden/make_scenario_synth.py): name -> (values, exact); exact
    columns (constants, coins) are float32 in agent order, the others sorted float16 (their marginal only)"""
    g = golden('scenario_synth')
    return {k[len(key) + 1:]: (g[k].astype(np.float32), g[k].dtype == np.float32) for k in g.files
            if k.startswith(key + '/') and '/' not in k[len(key) + 1:]}


def restated_cols(pos, wp, v0):
    cols = {'x': pos[:, 0], 'y': pos[:, 1], 'dx': wp[0, :, 0], 'dy': wp[0, :, 1], 'v0': v0}
    if wp.shape[0] > 1:
        cols.update(dx1=wp[1, :, 0], dy1=wp[1, :, 1])
    cols.update(x_side=np.sign(pos[:, 0]).astype(np.float32), abs_x=np.abs(pos[:, 0]))
    return cols


@pytest.mark.parametrize('name', ['crosswalk', 'basic_unit1', 'basic_unit2'])
def test_constant_coordinates_are_the_references(name):
    c = ref_cols(f'{name}/gen')
    sc = factory(name, uniform_desired_speed=False)
    L, W = np.float32(sc.length), np.float32(sc.width)
    u = lambda k: set(np.unique(c[k][0]).tolist())
    if name == 'crosswalk':
        assert c['y'][1] and c['dx'][1] and c['dy'][1] and c['x_side'][1]
        assert u('y') == {-W / 2, W / 2} and u('dx') == {-L / 2, L / 2} and u('dy') == {-W / 2, W / 2}
        assert u('x_side') == {-1.0, 1.0}
        assert np.array_equal(c['dx1'][0], c['dx'][0]) and np.array_equal(c['dy1'][0], c['dy'][0] * np.float32(3))
        assert np.array_equal(c['dx'][0], -c['x_side'][0] * L / 2)          # the walk crosses to the other side
        assert c['abs_x'][0].min() >= L / 2 and c['abs_x'][0].max() <= L / 2 + 3
        assert sc.fixed_spawn_rate == 5 * 0.08 and factory(name, time_unit=0.1).spawn_rate == 5 * 0.08
    elif name == 'basic_unit1':
        assert u('x') == {0.0} and u('dx') == {float(L)} and 'dx1' not in c
    else:
        assert u('x') == {0.0, float(L)} and u('dx') == {0.0, float(L)}
        assert np.array_equal(c['x'][0] == L, c['dx'][0] == 0)


def test_basic_unit3_streams_are_the_references():
    c1, c2 = ref_cols('basic_unit3/gen/g1'), ref_cols('basic_unit3/gen/g2')
    sc = factory('basic_unit3')
    L, W = np.float32(sc.length), np.float32(sc.width)
    assert (c1['x'][0] == 0).all() and (c1['dx'][0] == L).all() and (c2['y'][0] == 0).all() and (c2['dy'][0] == W).all()
    assert sc.spawn_rate == 5 * 0.08 and abs(sc.spawn_rate2 - 0.08) < 1e-12 and sc.spawn_cap2 == 8
    thr2 = sc.poisson_thresholds2()
    assert len(thr2) == 8 and thr2 == sorted(thr2)


@pytest.mark.parametrize('name,group', [('crosswalk', None), ('basic_unit1', None), ('basic_unit2', None),
                                        ('basic_unit3', 0), ('basic_unit3', 1)])
def test_restated_spawn_laws_have_the_references_support(name, group):
    sc = factory(name, uniform_desired_speed=False)
    n = 20000
    pos, vel, wp, v0 = R.spawn(sc, 5, np.arange(n), None if group is None else np.full(n, group))
    ref = ref_cols(f'{name}/gen' + ('' if group is None else f'/g{group + 1}'))
    mine = restated_cols(pos, wp, v0)
    for k, (r, exact) in ref.items():
        if exact:                                       # the constants and coins take the reference's values, no others
            assert set(np.unique(mine[k]).tolist()) == set(np.unique(r).tolist()), k
        elif k != 'v0':                                 # bounded coordinates within the reference's range (float16: 2^-11)
            span = max(float(r.max() - r.min()), 1e-6)
            assert mine[k].min() >= r.min() - 2e-3 * span and mine[k].max() <= r.max() + 2e-3 * span, k
    sc_min = np.float32(sc.speed_min) if sc.speed_clamp else -np.inf
    assert v0.min() >= sc_min and abs(float(np.mean(v0)) - float(np.mean(ref['v0'][0]))) < 0.02
    assert np.allclose(np.linalg.norm(vel, axis=1), np.abs(v0))


def test_rules_abi_checks_without_gpu():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    assert _lib.ABI_VERSION == 35 and L.piml_abi_version() == 35
    assert 'piml_scenario_step_rules' in _lib.SIGNATURES
    s, r = _lib.Scenario(), _lib.ScenarioRules()
    assert L.piml_scenario_step_rules(None, None, None, 1, None) == 1
    assert L.piml_scenario_step_rules(ctypes.byref(s), None, None, 1, None) == 1
    assert L.piml_scenario_step_rules(ctypes.byref(s), ctypes.byref(r), None, 1, None) == 1   # GC rule: capacity 0
    good = ops_scenario.scenario_rules(factory('crosswalk'))
    s.capacity, s.T, s.hist_width, s.F, s.D, s.dt, s.n_initial, s.spawn_cap = 8, 4, 2, 7, 2, 0.08, 2, 0

    def code(**kw):
        rr = _lib.ScenarioRules.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(rr, k, v)
        return L.piml_scenario_step_rules(ctypes.byref(s), ctypes.byref(rr), None, 1, None)
    assert code() == 1                                               # every buffer NULL
    for bad in ({'spawn_law': 9}, {'arrival_rule': 7}, {'arrival_rule': 0}, {'spawn_law': 0}, {'initial_velocity': 2},
                {'speed_clamp': -1}, {'spawn_cap2': 2}, {'spawn_law': 2, 'grid': 0}, {'spawn_law': 2, 'grid': 1}):
        assert code(**bad) == 1, bad
    s.D = 1
    assert code() == 1                                               # the crosswalk needs 2 waypoints
    sq = ops_scenario.scenario_rules(factory('four_directional_square'))
    assert sq.grid == 5 and [sq.square_grid[j] for j in range(5)] == factory('four_directional_square').square_grid.tolist()
    u3 = ops_scenario.scenario_rules(factory('basic_unit3'))
    assert u3.spawn_cap2 == 8 and u3.spawn_law == _lib.SPAWN_LAWS['unit3']


def test_rules_state_refuses_cpu_scenarios():
    from piml_amd import _lib, ops_scenario
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.scenario_state(factory('crosswalk'), 64, 10)
    assert torch.equal(factory('basic_unit1').obstacles, torch.zeros(0, 2))
