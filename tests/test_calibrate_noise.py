"""CPU: the track side of the statistics fit and the fluctuation term's constants without a GPU -- stats_objective's
arithmetic on hand-made TrackStats (the union of terms, the default weights, a NaN term, an unknown weight), the search of
calibrate_mlapm_to_stats moving An and noise_tau through `evaluate=` inside their bounds, its refusals, and the command
line."""
import math

import numpy as np
import pytest

INIT = {'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
TRACK_KEYS = ('heading_ac_max_diff', 'persistence_time_diff', 'msd_exponent_diff', 'acc_l1', 'mean_acceleration_diff',
              'straightness_l1', 'speed_l1', 'duration_l1')
WEIGHTED = ('heading_ac_max_diff', 'msd_exponent_diff', 'acc_l1', 'mean_acceleration_diff', 'straightness_l1')
N_LAGS, ACC_BINS = 64, 40


def tracks(ac=0.9, exponent=2.0, acc_bin=1, mean_acc=0.3, straight_bin=19, speed_bin=12, dur_bin=20, pairs=1000, falls=False):
    """one pooled member: a heading autocorrelation of `ac` at every lag (falling below 1 / e from lag 32 on with `falls`), an
    MSD tau^exponent, 1000 acceleration items in one bin with mean `mean_acc`, 100 tracks in one bin of each histogram"""
    from piml_amd.trackstats import Q, TrackStats
    lag = np.arange(1, N_LAGS + 1, dtype=np.float64)
    a = {}
    a['ac_n'] = np.full((1, N_LAGS), pairs, np.int64)
    level = np.where(lag >= 32, 0.1, ac) if falls else np.full(N_LAGS, ac)
    a['ac_sum'] = np.round(level * Q * pairs).astype(np.int64)[None]
    a['msd_n'] = np.full((1, N_LAGS), pairs, np.int64)
    a['msd_sum'] = np.round((lag * 0.08) ** exponent * Q * pairs).astype(np.int64)[None]
    a['msd_far'] = np.zeros((1, N_LAGS), np.int64)
    a['acc'] = np.zeros((1, ACC_BINS + 1), np.int64)
    a['acc'][0, acc_bin] = 1000
    a['acc_sum'] = np.array([int(round(mean_acc * Q * 1000))], np.int64)
    for name, bins, at in (('dur_hist', 60, dur_bin), ('speed_hist', 40, speed_bin), ('straight_hist', 20, straight_bin)):
        a[name] = np.zeros((1, 2, bins), np.int64)
        a[name][0, :, at] = 100
    a['straight_n'] = np.full((1, 2), 100, np.int64)
    a['straight_sum'] = np.full((1, 2), 95 * Q, np.int64)
    opts = dict(dt=0.08, v_min=0.1, n_lags=N_LAGS, d_max=64.0, acc_bin=0.25, acc_bins=ACC_BINS, speed_bin=0.1, speed_bins=40,
                dur_bin=1.0, dur_bins=60, straight_bins=20, frames=(0, 200))
    return TrackStats(a, opts)


def test_objective_keys_weights_and_bounds():
    from piml_amd import calibrate as C
    assert C.OBJECTIVE_KEYS['tracks'] == TRACK_KEYS
    assert C.TRACK_DEFAULT_WEIGHTS == {'persistence_time_diff': 0.0, 'speed_l1': 0.0, 'duration_l1': 0.0}
    assert C.NOISE_PARAM_NAMES == ('An', 'noise_tau')
    assert C.DEFAULT_BOUNDS['An'] == (0.0, None) and C.DEFAULT_BOUNDS['noise_tau'] == (0.0, None)
    assert C.DEFAULT_BOUNDS['tau'] == (1e-3, None) and C.DEFAULT_BOUNDS['Ag'] == (0.0, None)      # the others as they were
    assert C.DEFAULT_WEIGHTS == {'speed_ratio_diff': 0.0}


def test_stats_objective_track_side():
    from piml_amd.calibrate import stats_objective
    from piml_amd.trackstats import compare_track_stats
    ref = tracks()
    J, terms = stats_objective(tracks=tracks(), ref_tracks=ref)
    assert J == 0.0 and set(TRACK_KEYS) <= set(terms)
    assert math.isnan(terms['persistence_time_diff'])               # neither falls below 1 / e: NaN, and at weight 0 J is finite
    # the ensemble that walks along rulers: a higher autocorrelation, ballistic against tau^1.6, smaller accelerations in
    # another bin, straighter; another speed and duration bin, which do not count by default
    sim = tracks(ac=0.98, exponent=2.0, acc_bin=0, mean_acc=0.1, straight_bin=19, speed_bin=10, dur_bin=30)
    ref = tracks(ac=0.9, exponent=1.6, acc_bin=1, mean_acc=0.3, straight_bin=18)
    J, terms = stats_objective(tracks=sim, ref_tracks=ref)
    want = compare_track_stats(sim, ref, 50)
    assert set(terms) == set(want) and all(terms[k] == want[k] or (math.isnan(terms[k]) and math.isnan(want[k])) for k in want)
    assert terms['heading_ac_max_diff'] == pytest.approx(0.08, abs=1e-5) and terms['msd_exponent_diff'] == pytest.approx(0.4, abs=1e-4)
    assert terms['acc_l1'] == 2.0 and terms['straightness_l1'] == 2.0 and terms['speed_l1'] == 2.0 and terms['duration_l1'] == 2.0
    assert terms['mean_acceleration_diff'] == pytest.approx(-0.2, abs=1e-5)
    assert J == pytest.approx(sum(abs(terms[k]) for k in WEIGHTED), abs=1e-12)
    assert J == pytest.approx(0.08 + 0.4 + 2.0 + 0.2 + 2.0, abs=2e-4)
    # the weights: the scene's terms on, a law's term off
    Jw, _ = stats_objective(tracks=sim, ref_tracks=ref, weights={'speed_l1': 1.0, 'duration_l1': 0.5, 'acc_l1': 0.0})
    assert Jw == pytest.approx(J - 2.0 + 2.0 + 1.0, abs=1e-12)
    # a NaN term of non-zero weight: inf
    Jn, _ = stats_objective(tracks=sim, ref_tracks=ref, weights={'persistence_time_diff': 1.0})
    assert Jn == float('inf')
    few = tracks(pairs=10)                                          # below min_count: no valid lag, heading_ac_max_diff NaN
    Jf, tf = stats_objective(tracks=few, ref_tracks=ref)
    assert math.isnan(tf['heading_ac_max_diff']) and Jf == float('inf')
    # with both sides falling below 1 / e the persistence time is a number, and the weight switches it on
    a, b = tracks(falls=True), tracks(ac=0.6, falls=True)
    J0, t0 = stats_objective(tracks=a, ref_tracks=b)
    J1, t1 = stats_objective(tracks=a, ref_tracks=b, weights={'persistence_time_diff': 2.0})
    assert math.isfinite(t0['persistence_time_diff']) and t0['persistence_time_diff'] != 0
    assert J1 == pytest.approx(J0 + 2.0 * abs(t0['persistence_time_diff']), abs=1e-12)
    with pytest.raises(ValueError, match='unknown'):
        stats_objective(tracks=sim, ref_tracks=ref, weights={'heading_l1': 1.0})
    with pytest.raises(ValueError, match='track'):                  # one half of a side is no side
        stats_objective(tracks=sim)
    # next to another side: the sum of both, the union of the terms
    from test_calibrate_stats import crowd
    Jc, _ = stats_objective(crowd=crowd(1.25), ref_crowd=crowd(1.0))
    Jb, tb = stats_objective(crowd=crowd(1.25), ref_crowd=crowd(1.0), tracks=sim, ref_tracks=ref)
    assert Jb == pytest.approx(Jc + J, abs=1e-12) and 'fd_distance' in tb and 'acc_l1' in tb
    Jp, _ = stats_objective(crowd(1.25), None, crowd(1.0), None, None, 50, None, None, None, None, sim, ref)   # positionally
    assert Jp == Jb


def search(evaluate, fit=('An',), init=None, log=None, **kw):
    from piml_amd.calibrate import calibrate_mlapm_to_stats

    def ev(cands):
        if log is not None:
            log.append([dict(c) for c in cands])
        return evaluate(cands)
    kw = {'population': 8, 'generations': 8, **kw}
    return calibrate_mlapm_to_stats(None, None, version='GC', init={**INIT, 'An': 0.5} if init is None else init, fit=fit,
                                    evaluate=ev, **kw)


def test_search_moves_the_fluctuation_term_inside_its_bounds():
    log = []
    res = search(lambda cs: [(c['An'] - 1.0) ** 2 for c in cs], log=log, sigma=1.0)
    assert abs(res.params['An'] - 1.0) < abs(0.5 - 1.0) and res.final_loss < res.initial_loss == 0.25
    assert all(y <= x for x, y in zip(res.history, res.history[1:]))
    assert res.params['noise_tau'] == 0.0 and res.fit == ('An',)
    for g in log:
        for c in g:
            assert c['noise_tau'] == 0.0 and c['version'] == 'GC' and 'Aw' not in c and 'Ag' not in c
            assert {k: c[k] for k in INIT} == INIT
    # both move; noise_tau starts at its bound 0 (scale 1) and has to leave it
    log = []
    res = search(lambda cs: [(c['An'] - 1.0) ** 2 + (c['noise_tau'] - 0.4) ** 2 for c in cs], fit=('An', 'noise_tau'), log=log,
                 sigma=0.5, generations=12)
    assert abs(res.params['An'] - 1.0) < 0.5 and 0.0 < res.params['noise_tau'] and abs(res.params['noise_tau'] - 0.4) < 0.4
    assert min(c['noise_tau'] for g in log for c in g) >= 0.0 and min(c['An'] for g in log for c in g) >= 0.0
    # the optimum lies below the bounds: the search walks into 0 and never past it
    log = []
    res = search(lambda cs: [(c['An'] + 2.0) ** 2 + (c['noise_tau'] + 1.0) ** 2 for c in cs], fit=('An', 'noise_tau'),
                 init={**INIT, 'An': 0.5, 'noise_tau': 0.25}, log=log, sigma=2.0)
    ans = [c['An'] for g in log for c in g]
    taus = [c['noise_tau'] for g in log for c in g]
    assert min(ans) == 0.0 and min(taus) == 0.0 and res.params['An'] >= 0.0 and res.params['noise_tau'] >= 0.0
    # a fit of the pair law alone carries a fluctuation term in init through untouched
    res = search(lambda cs: [(c['A'] - 3.0) ** 2 for c in cs], fit=('A',), init={**INIT, 'An': 0.7, 'noise_tau': 0.3})
    assert res.params['An'] == 0.7 and res.params['noise_tau'] == 0.3 and res.params['A'] != INIT['A']
    # and without one, nothing of it appears
    res = search(lambda cs: [(c['A'] - 3.0) ** 2 for c in cs], fit=('A',), init=dict(INIT))
    assert 'An' not in res.params and 'noise_tau' not in res.params


def test_fluctuation_term_refusals():
    from piml_amd.calibrate import calibrate_mlapm_to_stats
    ev = lambda cs: [0.0] * len(cs)                                  # noqa: E731
    with pytest.raises(ValueError, match='fluctuation term has no default'):
        calibrate_mlapm_to_stats(None, None, init=dict(INIT), fit=('An',), evaluate=ev)
    with pytest.raises(ValueError, match='fluctuation term has no default'):
        calibrate_mlapm_to_stats(None, None, init=dict(INIT), fit=('noise_tau',), evaluate=ev)
    with pytest.raises(ValueError, match='fluctuation term has no default'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'noise_tau': 0.5}, fit=('A',), evaluate=ev)
    with pytest.raises(ValueError, match='An >= 0'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'An': -1.0}, fit=('A',), evaluate=ev)
    with pytest.raises(ValueError, match='noise_tau >= 0'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'An': 1.0, 'noise_tau': -0.1}, fit=('A',), evaluate=ev)
    with pytest.raises(ValueError, match='names of'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'An': 1.0}, fit=('An', 'noise_rho'), evaluate=ev)


def test_command_line(capsys):
    from piml_amd import calibrate as C
    a = C.get_args(['--data', 'clip.npy', '--match-stats', '--match', 'crowd,pairs,tracks', '--fit', 'An,noise_tau', '--init',
                    'An=0.5'])
    assert a.fit == ('An', 'noise_tau') and a.init == {'An': 0.5} and a.match == ('crowd', 'pairs', 'tracks')
    a = C.get_args(['--data', 'clip.npy', '--match-stats', '--fit', 'An', '--init', 'An=0.5,noise_tau=0.3'])
    assert a.match == ('crowd', 'pairs', 'tracks')                   # on by default with a fluctuation term
    a = C.get_args(['--data', 'clip.npy', '--match-stats', '--match', 'tracks'])
    assert a.match == ('tracks',) and a.fit == C.PARAM_NAMES          # the track statistics may be matched without the term
    assert C.get_args(['--data', 'clip.npy', '--match-stats']).match == ('crowd', 'pairs')       # as before
    for argv, word in ((['--data', 'clip.npy', '--fit', 'An', '--init', 'An=0.5'], 'fitted by --match-stats only'),
                       (['--data', 'clip.npy', '--init', 'noise_tau=0.5'], 'fitted by --match-stats only'),
                       (['--data', 'clip.npy', '--match-stats', '--fit', 'An'], 'has no default'),
                       (['--data', 'clip.npy', '--match-stats', '--init', 'noise_tau=0.5'], 'has no default'),
                       (['--data', 'clip.npy', '--match-stats', '--match', 'crowd,track'], '--match')):
        with pytest.raises(SystemExit) as ex:
            C.get_args(argv)
        assert ex.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
