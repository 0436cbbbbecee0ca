"""CPU: the preconditions of test_stats_runs_gpu.py and test_stats_grid_cap_gpu.py.  Every shape they use gives the run
length (stats_runs_shapes.py, from the constants in the kernels' sources) it was chosen for, with a member boundary -- for
pairs also a lag boundary -- strictly inside a run; the groups of the run = 1 oracle have run == 1; the grid-cap shapes ask
for more workgroups than the cap and their parts for no more; and the float64 restatements of the three mid-size cases
report an ambiguous share under the cap the run = 1 tests use."""
import pytest

import stats_runs_shapes as SH


def test_constants_are_read_from_the_sources():
    for prefix in ('PS', 'FS', 'OS'):
        assert SH.constant(prefix + '_MAX_RUN') >= 3 and SH.constant(prefix + '_TARGET_WG') >= 1
    for prefix in SH.SOURCES:
        assert SH.constant(prefix + '_MAX_GRID') >= 1
    with pytest.raises(ValueError):
        SH.constant('PS_NO_SUCH_CONSTANT')


def test_run_formula():
    """clamp(slices / TARGET_WG, 1, MAX_RUN), the division truncating, at its edges"""
    for run_of, prefix in ((SH.flow_run, 'FS'), (SH.obstacle_run, 'OS')):
        wg, top = SH.constant(prefix + '_TARGET_WG'), SH.constant(prefix + '_MAX_RUN')
        assert run_of(1, 1) == 1 and run_of(1, 2 * wg - 1) == 1 and run_of(2, wg) == 2 and run_of(1, 3 * wg - 1) == 2
        assert run_of(top, wg) == top and run_of(top + 5, wg) == top and run_of(0, 5) == 1
    wg = SH.constant('PS_TARGET_WG')
    assert SH.pair_offsets(10, (2, 5, 30)) == [0, 10, 18, 23, 23]
    assert SH.pair_run(1, wg, ()) == 1 and SH.pair_run(2, wg, ()) == 2 and SH.pair_run(2, wg, (wg,)) == 2
    assert SH.pair_run(1, wg, (1,)) == 1 and SH.pair_run(1, wg + 1, (1,)) == 2


@pytest.mark.parametrize('name', sorted(SH.MID) + ['long_' + k for k in sorted(SH.LONG)])
def test_shapes_have_their_run_and_boundaries_inside_runs(name):
    c = SH.LONG[name[5:]] if name.startswith('long_') else SH.MID[name]
    kind = SH.kind_of(name[5:] if name.startswith('long_') else name)
    S, T, lags = c['S'], c['T'], c['lags']
    run, pm = SH.run_of(kind, S, T, lags), SH.per_member(kind, T, lags)
    assert run == c['run'], (name, run)
    assert pm % run != 0 and SH.member_boundaries_inside_runs(kind, S, T, lags), name
    assert SH.runs_of(kind, S, T, lags) <= SH.constant(SH.PREFIX[kind] + '_MAX_GRID')      # one trip round the grid loop
    if kind == 'pairs':
        inside = SH.lag_boundaries_inside_runs(S, T, lags)
        assert {k for _, k in inside} == {1, 2}, name            # both lags with slices start inside a run somewhere
        if 400 in lags:                                          # the lag past the window has no slice
            off = SH.pair_offsets(T, lags)
            assert off[-1] == off[-2] and all(k != 3 for _, k in inside)
    if name.startswith('long_'):
        g = SH.run_one_group(kind, T, lags)
        assert g >= 1 and SH.run_of(kind, g, T, lags) == 1 and SH.run_of(kind, S % g or g, T, lags) == 1
        assert g < S


def test_pair_shape_arithmetic():
    """the numbers the cases were chosen by"""
    assert SH.pair_offsets(331, (1, 7)) == [0, 331, 661, 985] and 7 * 985 == 6895 and 985 % 3 == 1
    assert SH.pair_offsets(300, (1, 7, 400))[-1] == 892 and 892 % 64 == 60
    assert 701 % 3 == 2 and 950 % 3 == 2
    n = SH.pair_n_active(7, 24)
    assert sorted(n)[:2] == [0, 12] and n.count(24) == 5


def test_grid_cap_shapes():
    t = SH.TRACKS
    cap = SH.constant('TS_MAX_GRID')
    tracks = t['S'] * t['N']
    assert cap < tracks <= 2 * cap                               # some workgroups take a second track, none a third
    assert cap // t['N'] == t['S'] - 1 and cap % t['N'] == 0     # the second tracks are the last member's
    assert [b for _, b in t['halves']][-1] == t['S'] and t['halves'][0][0] == 0 and t['halves'][0][1] == t['halves'][1][0]
    assert all((b - a) * t['N'] <= cap for a, b in t['halves'])
    c = SH.CROWD
    cap = SH.constant('CD_MAX_GRID')
    assert cap < c['S'] * c['T'] <= 2 * cap and c['T'] <= cap    # one member alone stays below the cap
    assert cap // c['T'] == c['S'] - 1                           # the second slices are the last member's


@pytest.mark.parametrize('name', ['pairs', 'flow', 'obstacles'])
def test_mid_size_references_are_unambiguous_enough(name):
    kind = SH.kind_of(name)
    want = SH.mid_reference(name)
    share = SH.ambiguous_share(kind, want)
    total = want['n_items' if kind == 'obstacles' else 'n_pairs']
    print(f'\n[stats runs] {name} {SH.MID[name]}: {want["n_ambiguous"]} ambiguous of {total} ({share:.2e})')
    assert total > 100000 and share <= SH.CAP, share
