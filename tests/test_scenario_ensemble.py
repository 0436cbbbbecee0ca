"""CPU: the C ABI of piml_scenario_step_members (exported; its argument checks refuse before any launch) and the CLI's
--seeds parsing of `python -m piml_amd.simulate`."""
import ctypes

import pytest

INVALID = 1                                             # hipErrorInvalidValue


def _gc_descriptor():
    """A GC descriptor every check of piml_scenario_step accepts; its pointers are never dereferenced (nothing here
    reaches a launch)."""
    from piml_amd import _lib
    from piml_amd.scenarios import gc_scenario
    sc = gc_scenario()
    s = _lib.Scenario()
    for name, _ in _lib.Scenario._fields_[:23]:         # every buffer pointer: non-NULL, 8-aligned
        setattr(s, name, 0x1000)
    s.hist_width, s.F, s.D, s.E, s.P, s.R = 2, 7, 2, 7, 100, 100
    s.capacity, s.T, s.n_initial, s.route_max_iters, s.spawn_cap = 64, 10, 20, 16, 8
    s.dt, s.arrival_radius, s.speed_mean = 0.08, 1.0, 1.34
    for j, x in enumerate(sc.poisson_thresholds()):
        s.poisson_thresholds[j] = x
    return s


def test_library_exports_the_member_entry():
    from piml_amd import _lib
    L = _lib.lib()
    assert hasattr(L, 'piml_scenario_step_members')
    assert _lib.ABI_VERSION == 35 and L.piml_abi_version() == 35


@pytest.mark.parametrize('members', [0, -1, 65536])
def test_member_count_outside_1_to_65535_is_refused(members):
    from piml_amd import _lib
    seeds = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    s = _gc_descriptor()
    assert _lib.lib().piml_scenario_step_members(ctypes.byref(s), None, members, seeds, None, 1, None) == INVALID


def test_null_seeds_and_the_single_entries_checks_are_refused():
    from piml_amd import _lib
    L = _lib.lib()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    s = _gc_descriptor()
    assert L.piml_scenario_step_members(ctypes.byref(s), None, 2, None, None, 1, None) == INVALID
    assert L.piml_scenario_step_members(None, None, 2, seeds, None, 1, None) == INVALID
    assert L.piml_scenario_step_members(ctypes.byref(s), None, 2, seeds, None, 0, None) == INVALID     # no a_next
    s.capacity = 0
    assert L.piml_scenario_step_members(ctypes.byref(s), None, 2, seeds, None, 1, None) == INVALID
    s = _gc_descriptor()
    s.poisson_thresholds[3] = 0                                                                        # decreasing
    assert L.piml_scenario_step_members(ctypes.byref(s), None, 2, seeds, None, 1, None) == INVALID
    s = _gc_descriptor()
    r = _lib.ScenarioRules()
    r.spawn_law, r.arrival_rule = _lib.SPAWN_LAWS['crosswalk'], _lib.ARRIVAL_RULES['gc']                # law / rule clash
    assert L.piml_scenario_step_members(ctypes.byref(s), ctypes.byref(r), 2, seeds, None, 1, None) == INVALID
    r.arrival_rule, r.spawn_cap2 = _lib.ARRIVAL_RULES['radius'], 1                                      # cap2 not UNIT3
    assert L.piml_scenario_step_members(ctypes.byref(s), ctypes.byref(r), 2, seeds, None, 1, None) == INVALID


def test_seeds_parsing():
    from piml_amd.simulate import get_args, parse_seeds
    assert parse_seeds('0:4') == [0, 1, 2, 3]
    assert parse_seeds('3,5,11') == [3, 5, 11]
    own, _ = get_args(['--seeds', '0:4', '--out', 'clip_{seed}.npy'])
    assert own.seeds == [0, 1, 2, 3]
    own, _ = get_args(['--seeds', '3,5,11', '--out', 'clip_{seed}.npy'])
    assert own.seeds == [3, 5, 11]
    own, _ = get_args(['--seed', '7'])
    assert own.seed == 7 and own.seeds is None
    for bad in ('4:4', 'a,b', ''):
        with pytest.raises(ValueError):
            parse_seeds(bad)


@pytest.mark.parametrize('argv', [['--seed', '1', '--seeds', '0:3', '--out', 'c_{seed}.npy'],   # --seed and --seeds clash
                                  ['--seeds', '0:3', '--out', 'clip.npy'],                      # no {seed} in the pattern
                                  ['--seeds', '3:1', '--out', 'c_{seed}.npy']])                 # no seed at all
def test_seeds_cli_errors(argv):
    from piml_amd.simulate import get_args
    with pytest.raises(SystemExit) as ex:
        get_args(argv)
    assert ex.value.code != 0
