"""CPU: time-to-collision and pair-distance statistics (piml_amd.pairstats) without a GPU -- the numpy restatement
(pairstats_ref.py) on hand cases, option validation, the derived quantities on synthetic counts (g(tau), E(tau) and its
exponent, g(r), overlap rate), pooling, merging, JSON, compare_pair_stats, the command line's parsing, and the C entry's
exports and argument checks (rejected before any HIP call)."""
import json
import math

import numpy as np
import pytest

import pairstats_ref as REF

R = 0.5


def _one_frame(P, V, M=None, **kw):
    P = np.asarray(P, np.float32)[None]
    V = np.asarray(V, np.float32)[None]
    M = np.ones(P.shape[:2], np.float32) if M is None else np.asarray(M, np.float32)[None]
    return REF.pair_stats(P, V, M, lags=(), **kw)


def test_head_on_pair():
    D, u = 3.03, 1.0
    st = _one_frame([[0, 0], [D, 0]], [[u, 0], [-u, 0]])
    tau = (D - R) / (2 * u)
    e = REF.classify(np.array([[0, 0]], np.float32), np.array([[u, 0]], np.float32), np.array([[D, 0]], np.float32),
                     np.array([[-u, 0]], np.float32), np.zeros((1, 1), bool), R, None, 0.1, 100, 0.05, 100, np.float64)
    assert e['course'][0, 0] and e['tau'][0, 0] == pytest.approx(tau, rel=1e-6)
    tb, db = int(tau / np.float32(0.1)), int(np.float32(D) / np.float32(0.05))
    assert st['focal'].tolist() == [[2]] and st['pairs'].tolist() == [[2]] and st['overlap'].tolist() == [[0]]
    assert st['ttc'][0, 0, tb] == 2 and st['ttc'].sum() == 2
    assert st['dist'][0, 0, db] == 2 and st['dist'].sum() == 2
    assert st['nn'][0, db] == 2 and st['min_ttc'][0, tb] == 2
    assert st['n_ambiguous'] == 0 and st['n_pairs'] == 2
    for k in REF.OUTPUTS:
        assert np.array_equal(st['f32'][k], st[k]), k


def test_crossing_receding_overlapping():
    # crossing: they meet at (5, 0) at t = 5; |d + w t| = R at t = 5 - sqrt(R^2 / 2)
    st = _one_frame([[0, 0], [5, -5]], [[1, 0], [0, 1]])
    tau = 5 - math.sqrt(R * R / 2)
    assert st['ttc'][0, 0, int(tau / 0.1)] == 2 and st['ttc'].sum() == 2
    # receding: b > 0, no collision course; the distance still counts, the smallest tau is 'none'
    st = _one_frame([[0, 0], [2.02, 0]], [[-1, 0], [1, 0]])
    assert st['ttc'].sum() == 0 and st['pairs'][0, 0] == 2 and st['dist'][0, 0, 40] == 2 and st['min_ttc'][0, 100] == 2
    # parallel at 1 m: b = 0, never closer
    st = _one_frame([[0, 0], [0, 1]], [[1, 0], [1, 0]])
    assert st['ttc'].sum() == 0 and st['min_ttc'][0, 100] == 2
    # passing at 2 m: b < 0 but disc < 0 (the closest approach stays outside R)
    st = _one_frame([[0, 0], [5, 2]], [[1, 0], [-1, 0]])
    assert st['ttc'].sum() == 0 and st['min_ttc'][0, 100] == 2
    # overlapping: no tau; overlap counts both ordered pairs; min_ttc skips the pair
    st = _one_frame([[0, 0], [0.3, 0]], [[1, 0], [-1, 0]])
    assert st['overlap'][0, 0] == 2 and st['ttc'].sum() == 0 and st['min_ttc'][0, 100] == 2 and st['nn'][0, 6] == 2
    # r_max skips the pair entirely
    st = _one_frame([[0, 0], [3.03, 0]], [[1, 0], [-1, 0]], r_max=3.0)
    assert st['pairs'][0, 0] == 0 and st['ttc'].sum() == 0 and st['nn'][0, 100] == 2 and st['min_ttc'][0, 100] == 2


def test_participants_box_and_slot_exclusion():
    # agent 2 has a NaN velocity, agent 3 is absent, agent 4 has a mask of 0.5: only 0 and 1 take part
    P = [[0, 0], [2, 0], [1, 0.2], [1, -0.2], [0.5, 0.5]]
    V = [[1, 0], [-1, 0], [np.nan, 0], [0, 0], [0, 0]]
    st = _one_frame(P, V, M=[1, 1, 1, 0, 0.5])
    assert st['focal'][0, 0] == 2 and st['pairs'][0, 0] == 2
    st = _one_frame(P, V, M=[1, 1, 1, 0, 0.5], box=(-1, 1, -1, 1))                # agent 1 (x = 2) is not focal
    assert st['focal'][0, 0] == 1 and st['pairs'][0, 0] == 1 and st['nn'].sum() == 1
    # lags: a lone agent never pairs with its own future; two agents give two ordered pairs per slice
    T = 6
    P1 = np.zeros((T, 1, 2), np.float32)
    V1 = np.zeros((T, 1, 2), np.float32)
    st = REF.pair_stats(P1, V1, np.ones((T, 1)), lags=(1, 3, 9))
    assert st['focal'].tolist() == [[6, 5, 3, 0]] and st['pairs'].sum() == 0
    P2 = np.stack([np.zeros((T, 2)), np.full((T, 2), 1.0)], 1).astype(np.float32)
    st = REF.pair_stats(P2, np.zeros_like(P2), np.ones((T, 2)), lags=(1, 3, 9), frames=(1, 6))
    assert st['focal'].tolist() == [[10, 8, 4, 0]] and st['pairs'].tolist() == [[10, 8, 4, 0]]
    assert st['nn'].sum() == 10 and st['ttc'].sum() == 0


def test_options_are_validated():
    from piml_amd.pairstats import check_options
    assert check_options() == ((64, 128, 192), None, None)
    assert check_options(lags=[], box=(0, 1, 0, 2), frames=(2, 9), T=10) == ((), (0.0, 1.0, 0.0, 2.0), (2, 9))
    for bad in (dict(radius=0), dict(radius=float('nan')), dict(tau_bin=0), dict(r_bin=-1), dict(tau_bins=0),
                dict(tau_bins=257), dict(r_bins=2.5), dict(r_max=0), dict(r_max=float('inf')), dict(lags=(0, 5)),
                dict(lags=(5, 5)), dict(lags=(6, 5)), dict(lags=tuple(range(1, 10))), dict(lags=(1.5,)),
                dict(box=(0, 0, 0, 1)), dict(box=(0, 1, 0)), dict(box=(0, float('inf'), 0, 1)),
                dict(frames=(3, 3), T=10), dict(frames=(-1, 3), T=10), dict(frames=(0, 11), T=10)):
        with pytest.raises(ValueError):
            check_options(**bad)


def _stats(ttc0, ttc_s, pairs0=10 ** 12, pairs_s=10 ** 12, dist0=None, dist_s=None, overlap0=0, focal0=1, nn=None,
           tau_bin=0.1, r_bin=0.05):
    from piml_amd.pairstats import PairStats
    TB = len(ttc0)
    dist0 = np.zeros(4, np.int64) if dist0 is None else np.asarray(dist0)
    dist_s = np.zeros_like(dist0) if dist_s is None else np.asarray(dist_s)
    RB = len(dist0)
    arrays = dict(focal=[[focal0, 1]], pairs=[[pairs0, pairs_s]], overlap=[[overlap0, 0]], ttc=[[ttc0, ttc_s]],
                  dist=[[dist0, dist_s]], nn=[np.zeros(RB + 1, np.int64) if nn is None else nn],
                  min_ttc=[np.zeros(TB + 1, np.int64)])
    return PairStats(arrays, dict(radius=0.5, lags=(64,), tau_bin=tau_bin, tau_bins=TB, r_bin=r_bin, r_bins=RB,
                                  r_max=None, box=None, frames=(0, 750)))


def test_energy_power_law_is_recovered():
    TB = 40
    tau = (np.arange(TB) + 0.5) * float(np.float32(0.1))
    scr = np.full(TB, 10 ** 15, np.int64)
    lag0 = np.rint(1e15 * np.exp(-tau ** -2.0)).astype(np.int64)
    st = _stats(lag0, scr)
    g = st.g_tau(min_count=50)
    ok = np.isfinite(g)
    assert ok[2:].all() and not ok[0]                          # exp(-100) * 1e15 < 50 at the first centre
    np.testing.assert_allclose(st.interaction_energy()[2:], tau[2:] ** -2.0, rtol=1e-6)
    p, n = st.energy_exponent(tau_range=(0.2, 2.5))
    assert n == 23 and abs(p + 2.0) < 1e-6
    p3, _ = _stats(np.rint(1e15 * np.exp(-0.5 * tau ** -3.0)).astype(np.int64), scr).energy_exponent()
    assert abs(p3 + 3.0) < 1e-6
    assert math.isnan(st.energy_exponent(tau_range=(10, 20))[0])
    # the densities: counts over (pairs x bin width)
    np.testing.assert_allclose(st.ttc_density(0), lag0 / (1e12 * float(np.float32(0.1))))
    np.testing.assert_allclose(st.scrambled_ttc_density(), scr / (1e12 * float(np.float32(0.1))))


def test_g_r_overlap_rate_and_nn():
    st = _stats(np.zeros(3, np.int64), np.zeros(3, np.int64), pairs0=1000, pairs_s=3000, dist0=[10, 100, 200, 40],
                dist_s=[300, 300, 600, 30], overlap0=7, focal0=20, nn=[0, 5, 10, 0, 5])
    g = st.g_r(min_count=50)
    assert math.isnan(g[0]) and math.isnan(g[3])
    np.testing.assert_allclose(g[1:3], [0.1 / 0.1, 0.2 / 0.2])
    assert st.overlap_rate() == pytest.approx(7 / 20)
    np.testing.assert_allclose(st.nn_density(), np.array([0, 5, 10, 0]) / (20 * float(np.float32(0.05))))
    assert np.isnan(st.g_tau()).all()


def test_pooled_merge_json_and_compare(tmp_path):
    from piml_amd.pairstats import PairStats, compare_pair_stats, merge
    rng = np.random.default_rng(0)
    S, K1, TB, RB = 3, 3, 5, 4
    arrays = dict(focal=rng.integers(0, 100, (S, K1)), pairs=rng.integers(1000, 2000, (S, K1)),
                  overlap=rng.integers(0, 10, (S, K1)), ttc=rng.integers(0, 500, (S, K1, TB)),
                  dist=rng.integers(0, 500, (S, K1, RB)), nn=rng.integers(0, 30, (S, RB + 1)),
                  min_ttc=rng.integers(0, 30, (S, TB + 1)))
    opts = dict(radius=0.5, lags=(2, 4), tau_bin=0.1, tau_bins=TB, r_bin=0.05, r_bins=RB, r_max=None, box=(0.0, 1.0, 0.0, 1.0),
                frames=(0, 10))
    st = PairStats(arrays, opts)
    assert st.members == 3 and st.member(1).ttc.tolist() == [arrays['ttc'][1].tolist()]
    p = st.pooled()
    for k in arrays:
        assert np.array_equal(p.__dict__[k][0], arrays[k].sum(0)), k
    m = merge([st.member(0), st.member(1), st.member(2)])
    for k in arrays:
        assert np.array_equal(getattr(m, k), getattr(p, k)), k
    assert PairStats.merge([st, st]).focal.tolist() == [(2 * arrays['focal'].sum(0)).tolist()]
    other = PairStats(arrays, {**opts, 'frames': (0, 20)})
    assert merge([st, other]).options['frames'] is None
    with pytest.raises(ValueError):
        merge([st, PairStats(arrays, {**opts, 'lags': (2, 5)})])
    d = st.to_json(str(tmp_path / 'p.json'))
    back = PairStats.from_json(str(tmp_path / 'p.json'))
    for k in arrays:
        assert np.array_equal(getattr(back, k), getattr(st, k)), k
    assert back.options == st.options and json.loads(json.dumps(d)) == d
    with pytest.raises(ValueError):
        PairStats.from_json({**d, 'version': 99})
    c = compare_pair_stats(st, back, min_count=1)
    assert c['ttc_l1'] == 0.0 and c['nn_l1'] == 0.0 and c['g_tau_max_diff'] == 0.0 and c['g_tau_bins'] == TB
    assert c['overlap_rate_diff'] == 0.0 and (c['energy_exponent_diff'] == 0.0 or math.isnan(c['energy_exponent_diff']))
    c2 = compare_pair_stats(st.member(0), st.member(1), min_count=1)
    assert c2['ttc_l1'] > 0 and c2['nn_l1'] > 0
    with pytest.raises(ValueError):
        compare_pair_stats(st, PairStats(arrays, {**opts, 'tau_bin': 0.2}))


def test_cli_parsing():
    from piml_amd import pairstats
    a = pairstats.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'r.npy', '--box', 'auto', '--frames', '3:400',
                            '--lags', '8,16', '--r_max', '4', '--out', 'o.json'])
    assert a.data == ['a.npy', 'b.npy'] and a.ref == 'r.npy' and a.box == 'auto' and a.frames == (3, 400)
    assert a.lags == (8, 16) and a.r_max == 4.0 and a.radius == 0.5 and a.tau_bins == 100 and a.out == 'o.json'
    d = pairstats.get_args(['--data', 'a.npy', '--box', '5,25,15,35'])
    assert d.box == (5.0, 25.0, 15.0, 35.0) and d.lags == (64, 128, 192) and d.frames is None
    assert pairstats.get_args(['--data', 'a.npy', '--lags', '']).lags == ()
    for bad in (['--data', 'a.npy', '--lags', '5,3'], ['--data', 'a.npy', '--lags', '0'], ['--data', 'a.npy', '--box', '1,2'],
                ['--data', 'a.npy', '--frames', '5:5'], ['--data', 'a.npy', '--tau_bins', '300'], ['--lags', '1']):
        with pytest.raises(SystemExit):
            pairstats.get_args(bad)


def test_simulate_accepts_pair_stats_flag():
    from piml_amd import simulate
    own, _ = simulate.get_args(['--seeds', '0:2', '--pair-stats', 'p.json', '--frames', '40'])
    assert own.pair_stats == 'p.json' and own.stats is None and own.seeds == [0, 1]
    own, _ = simulate.get_args(['--frames', '40'])
    assert own.pair_stats is None


def test_library_exports_and_rejects_bad_arguments():
    import ctypes
    from test_abi import declared_symbols
    from piml_amd import _lib
    assert {'piml_pair_stats', 'piml_pair_stats_workspace_bytes'} <= set(declared_symbols())
    assert {'piml_pair_stats', 'piml_pair_stats_workspace_bytes'} <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert hasattr(L, 'piml_pair_stats') and hasattr(L, 'piml_pair_stats_workspace_bytes')
    fake = 1 << 20          # never dereferenced: every call below is refused before any HIP call
    good = (ctypes.c_int * 3)(4, 8, 12)

    def call(S=1, T=2, N=3, t0=0, t1=2, lags=good, K=3, R=0.5, rmax=0.0, box=0, x1=1., y0=0., tb=0.1, TB=4, rb=0.05,
             RB=4, nul=fake, wsb=1 << 20):
        lp = None if lags is None else ctypes.addressof(lags)
        return L.piml_pair_stats(nul, fake, fake, None, S, T, N, t0, t1, lp, K, R, rmax, box, 0., x1, y0, 1., tb, TB, rb,
                                 RB, fake, fake, fake, fake, fake, fake, fake, fake, wsb, None)
    for bad in (dict(S=0), dict(T=0), dict(N=0), dict(N=65537), dict(t0=2), dict(t1=3), dict(t0=-1), dict(K=9),
                dict(K=-1), dict(lags=None), dict(lags=(ctypes.c_int * 3)(4, 4, 12)), dict(lags=(ctypes.c_int * 3)(0, 4, 8)),
                dict(R=0.0), dict(R=float('inf')), dict(rmax=float('nan')), dict(tb=0.0), dict(TB=0), dict(TB=257),
                dict(rb=-1.0), dict(RB=257), dict(box=1, x1=0.), dict(box=1, y0=2.), dict(nul=None), dict(wsb=8)):
        assert call(**bad) == 1, bad
    assert L.piml_pair_stats_workspace_bytes(2, 3, 5, 7) == 2 * (3 * 4 + 4 * 5 + 4 * 7 + 8 + 6) * 8
    assert L.piml_pair_stats_workspace_bytes(2, -1, 5, 7) == -1
