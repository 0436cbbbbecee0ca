"""CPU: track statistics (piml_amd.trackstats) without a GPU -- the numpy restatement (trackstats_ref.py) on hand-counted
tracks and against itself on the random tracks of the GPU tests (with their ambiguous share), option validation, the host
histograms, the derived quantities on synthetic counts, pooling, merging, JSON, compare_track_stats, the command lines'
parsing, and the C entry's exports, constants and argument checks (refused before any HIP call)."""
import io
import math
import os
import re

import numpy as np
import pytest

import trackstats_ref as REF
from conftest import REPO

Q = REF.Q
STEP = 0.125                                  # metres per frame along x: exact in float32, as are its multiples near 10


def _tracks(cols, **kw):
    """cols: per track a list of T positions (None: absent) -> the restatement's result and its inputs"""
    T = len(cols[0])
    P = np.zeros((1, T, len(cols), 2), np.float32)
    M = np.zeros((1, T, len(cols)), np.float32)
    for n, col in enumerate(cols):
        for t, p in enumerate(col):
            if p is not None:
                P[0, t, n], M[0, t, n] = p, 1.0
    return REF.track_stats(P, M, **kw), P, M


def _hists(st, Tp, dt=0.08, **kw):
    from piml_amd.trackstats import track_histograms
    return track_histograms(st, Tp, dt, **kw)


def _same_in_both_runs(st):
    assert st['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(st[k], st['f32'][k]), k


def test_straight_tracks_along_x_and_oblique():
    """constant velocity (0.125, 0) and (0.09375, 0.125) = 0.15625 (0.6, 0.8) per frame over 20 frames: every heading pair
    is parallel, MSD(L) = (l L)^2, no acceleration, net = path"""
    T, NL = 20, 8
    cols = [[(10.0 + STEP * t, 3.0) for t in range(T)], [(10.0 + 0.09375 * t, 6.0 + 0.125 * t) for t in range(T)]]
    st, _, _ = _tracks(cols, n_lags=NL)
    _same_in_both_runs(st)
    for L in range(1, NL + 1):
        assert st['ac_n'][0, L - 1] == 2 * (T - 1 - L) and st['ac_sum'][0, L - 1] == 2 * (T - 1 - L) * Q      # A Q = Q exactly
        assert st['msd_n'][0, L - 1] == 2 * (T - L) and st['msd_far'][0, L - 1] == 0
        # (0.125 L)^2 Q = 2^14 L^2 and (0.15625 L)^2 Q = 25600 L^2 are integers
        assert st['msd_sum'][0, L - 1] == (T - L) * (16384 + 25600) * L * L
    assert st['acc'][0].tolist() == [2 * (T - 2)] + [0] * 40 and st['acc_sum'][0] == 0
    assert st['trk_frames'][0].tolist() == [T, T] and st['trk_steps'][0].tolist() == [T - 1, T - 1]
    assert st['trk_first'][0].tolist() == [0, 0] and st['trk_last'][0].tolist() == [T - 1, T - 1]
    assert st['trk_path'][0].tolist() == [(T - 1) * Q // 8, (T - 1) * 163840] == st['trk_net'][0].tolist()
    h = _hists(st, T)
    assert h['straight_hist'][0, 0].tolist() == [0] * 19 + [2] and h['straight_n'][0].tolist() == [2, 0]
    assert h['straight_sum'][0, 0] == 2 * Q and h['straight_hist'][0, 1].sum() == 0       # neither track is complete
    # 0.125 / 0.08 = 1.5625 m/s and 0.15625 / 0.08 = 1.953 m/s; 20 frames x 0.08 s = 1.6 s
    assert h['speed_hist'][0, 0, 15] == 1 and h['speed_hist'][0, 0, 19] == 1 and h['dur_hist'][0, 0, 1] == 2


def test_regular_polygon_at_constant_speed():
    """one vertex of a regular 16-gon of radius 4 m per frame: the heading turns by 2 pi / 16 per step, so A(L) =
    cos(L 2 pi / 16), and |u' - u| = 2 l sin(pi / 16) for every item.  The float32 vertices are off the circle by up to half
    an ulp of 4 m (2.4e-7 m) per coordinate, a step by 6.8e-7 m, its heading by 6.8e-7 / l = 4.4e-7 rad, a heading pair's
    cosine by 8.7e-7, 0.92 units at Q; with the rounding to an integer, 2 units per pair against the exact cosine."""
    K, R, T, NL = 16, 4.0, 40, 20
    ang = 2 * math.pi / K
    cols = [[(R * math.cos(ang * t), R * math.sin(ang * t)) for t in range(T)]]
    st, _, _ = _tracks(cols, n_lags=NL, acc_bin=4.0, acc_bins=40)
    assert st['n_ambiguous'] == 0
    REF.check(st['f32'], st, 'polygon')
    for run in (st, st['f32']):
        for L in range(1, NL + 1):
            n = T - 1 - L
            assert run['ac_n'][0, L - 1] == n
            assert abs(run['ac_sum'][0, L - 1] - n * math.cos(L * ang) * Q) <= 2 * n, L
        l = 2 * R * math.sin(ang / 2)
        a = 2 * l * math.sin(ang / 2) / 0.08 ** 2          # 95.15 m/s^2: bin 23 of 4 m/s^2
        assert int(a / 4.0) == 23 and abs(a / 4.0 - 23.5) < 0.4
        assert run['acc'][0, 23] == T - 2 and run['acc'][0].sum() == T - 2
        assert run['acc_sum'][0] == pytest.approx((T - 2) * a * Q, rel=1e-5)
        assert run['trk_path'][0, 0] == pytest.approx((T - 1) * l * Q, rel=1e-6)


def test_out_and_back():
    """10 steps out along x and 10 back: pairs that straddle the turn are anti-parallel, the net displacement is zero"""
    T = 21
    cols = [[(10.0 + STEP * min(t, T - 1 - t), 2.0) for t in range(T)]]
    st, _, _ = _tracks(cols, n_lags=12)
    _same_in_both_runs(st)
    for L in range(1, 13):
        pairs = [(t, t + L) for t in range(T - 1) if t + L <= T - 2]
        want = sum(1 if (a < 10) == (b < 10) else -1 for a, b in pairs)
        assert st['ac_n'][0, L - 1] == len(pairs) and st['ac_sum'][0, L - 1] == want * Q
    assert st['ac_sum'][0, 0] == 17 * Q and st['ac_sum'][0, 9] == -10 * Q          # A(1) = 17 / 19, A(10) = -1
    assert st['trk_net'][0, 0] == 0 and st['trk_path'][0, 0] == 20 * Q // 8
    # the turn is the one item with an acceleration: |u' - u| = 0.25 m, a = 39.06 m/s^2, beyond the 10 m/s^2 of the bins
    assert st['acc'][0, 0] == T - 3 and st['acc'][0, 40] == 1 and st['acc_sum'][0] == 0
    h = _hists(st, T)
    assert h['straight_hist'][0, 0].tolist() == [1] + [0] * 19 and h['straight_sum'][0, 0] == 0


def test_track_with_a_hole():
    """present at frames 0..5 and 8..14 at constant velocity: steps 0..4 and 8..13; pairs across the hole count when both ends
    are there"""
    T = 15
    there = set(range(0, 6)) | set(range(8, 15))
    cols = [[(10.0 + STEP * t, 1.0) if t in there else None for t in range(T)]]
    st, _, _ = _tracks(cols, n_lags=14)
    _same_in_both_runs(st)
    steps = {t for t in there if t + 1 in there}
    assert steps == {0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13} and st['trk_steps'][0, 0] == 11 and st['trk_frames'][0, 0] == 13
    for L in range(1, 15):
        n_ac = sum(1 for t in steps if t + L in steps)
        n_msd = sum(1 for t in there if t + L in there)
        assert st['ac_n'][0, L - 1] == n_ac and st['ac_sum'][0, L - 1] == n_ac * Q, L
        assert st['msd_n'][0, L - 1] == n_msd and st['msd_sum'][0, L - 1] == n_msd * 16384 * L * L, L
    assert st['ac_n'][0, :3].tolist() == [9, 7, 5] and st['msd_n'][0, :3].tolist() == [11, 9, 8]
    assert st['msd_n'][0, 13] == 1 and st['ac_n'][0, 13] == 0          # frames 0 and 14; no step starts at 14
    assert st['acc'][0, 0] == 4 + 5 and st['trk_first'][0, 0] == 0 and st['trk_last'][0, 0] == 14
    assert st['trk_path'][0, 0] == 11 * Q // 8 and st['trk_net'][0, 0] == 14 * Q // 8
    # the same track inside a window: the indices are the window's
    P = np.zeros((1, T + 4, 1, 2), np.float32)
    M = np.zeros((1, T + 4, 1), np.float32)
    for t in there:
        P[0, t + 3, 0], M[0, t + 3, 0] = (10.0 + STEP * t, 1.0), 1.0
    win = REF.track_stats(P, M, n_lags=14, frames=(3, T + 3))
    for k in REF.OUTPUTS:
        assert np.array_equal(win[k], st[k]), k
    cut = REF.track_stats(P, M, n_lags=14, frames=(5, 12))              # frames 2..5 and 8 of the track
    assert cut['trk_frames'][0, 0] == 5 and cut['trk_first'][0, 0] == 0 and cut['trk_last'][0, 0] == 6
    assert cut['trk_steps'][0, 0] == 3 and cut['ac_n'][0, :7].tolist() == [2, 1, 0, 0, 0, 0, 0]
    assert cut['msd_n'][0, :7].tolist() == [3, 2, 2, 1, 1, 1, 0]


def test_standing_agent_far_pairs_and_who_takes_part():
    T = 12
    still = [(7.0, 7.0)] * T
    walk = [(10.0 + STEP * t, 3.0) for t in range(T)]
    st, P, M = _tracks([still, walk], n_lags=10, d_max=0.9)
    _same_in_both_runs(st)
    # the standing agent: steps but no mover; MSD 0; it counts in trk_frames.  The walker alone moves: 0.125 L < 0.9 up to L = 7
    for L in range(1, 11):
        near = L <= 7
        assert st['ac_n'][0, L - 1] == max(T - 1 - L, 0)
        assert st['msd_n'][0, L - 1] == (T - L) * (2 if near else 1) and st['msd_far'][0, L - 1] == (0 if near else T - L)
        assert st['msd_sum'][0, L - 1] == (16384 * L * L * (T - L) if near else 0)
    assert st['trk_frames'][0].tolist() == [T, T] and st['trk_steps'][0].tolist() == [T - 1, T - 1]
    assert st['trk_path'][0, 0] == 0 and st['trk_net'][0, 0] == 0 and st['acc'][0, 0] == 2 * (T - 2)
    h = _hists(st, T)
    assert h['straight_n'][0].tolist() == [1, 0] and h['speed_hist'][0, 0, 0] == 1 and h['dur_hist'][0, 0].sum() == 2
    # who takes part: a mask of 0.5, NaN, inf, a coordinate of 65536 take the frame out; n_active takes the slot out
    P2, M2 = np.repeat(P, 5, 2), np.repeat(M, 5, 2)
    P2[0, :, 0::2] = P[0, :, 1:2]                          # every column walks
    P2[0, :, 1::2] = P[0, :, 1:2]
    M2[0, 4, 0] = 0.5
    P2[0, 4, 1, 0] = np.nan
    P2[0, 4, 2, 1] = np.inf
    P2[0, 4, 3, 0] = -65536.0
    P2[0, 4, 4, 0] = 65535.0                                # below the bound: takes part, 65525 m away for one frame
    part = REF.track_stats(P2[:, :, :6], M2[:, :, :6], n_lags=3, n_active=[5])
    assert part['trk_frames'][0].tolist() == [T - 1] * 4 + [T, 0] and part['trk_steps'][0].tolist() == [T - 3] * 4 + [T - 1, 0]
    assert part['trk_first'][0].tolist() == [0] * 5 + [-1] and part['trk_last'][0].tolist() == [T - 1] * 5 + [-1]
    assert part['msd_far'][0].tolist() == [2, 2, 2] and part['acc'][0, 40] == 3
    assert part['msd_n'][0, 0] == 4 * (T - 3) + T - 3
    full = REF.track_stats(P2[:, :, :6], M2[:, :, :6], n_lags=3)
    assert full['trk_frames'][0, 5] == T and full['msd_n'][0, 0] == part['msd_n'][0, 0] + T - 1


@pytest.mark.parametrize('N,S,T,NL,centred', [(300, 2, 40, 16, False), (65, 3, 300, 130, False), (1500, 1, 12, 32, False),
                                              (7, 2, 1024 + 1 + 64, 64, False), (65, 3, 300, 130, True),
                                              (300, 2, 40, 16, True)])
def test_restatement_runs_agree_on_random_tracks(N, S, T, NL, centred):
    """the float32 run lies within the float64 run's tolerances, and the ambiguous share of the generator the GPU tests use
    stays below their cap, per kind of item"""
    P, M = REF.random_tracks(S, T, N, seed=N + T, centred=centred)
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    for kw in (dict(n_lags=NL), dict(n_lags=NL, frames=(1, T), n_active=n_active, v_min=0.3, acc_bin=0.4, acc_bins=12,
                                     d_max=3.0)):
        st = REF.track_stats(P, M, **kw)
        print(N, S, T, sorted(kw), st['n_items'], st['kinds'], st['f32_deviation'])
        for k in REF.OUTPUTS:
            assert (np.abs(st['f32'][k] - st[k]) <= st['tol'][k]).all(), k
        for kind, (n, amb) in st['kinds'].items():
            assert amb <= 1e-3 * max(n, 1) + 1, (kind, n, amb)
        assert st['ac_n'].sum() > 0 and st['msd_n'].sum() > 0 and st['acc'].sum() > 0
        if 'd_max' in kw and T >= 40:
            assert st['msd_far'].sum() > 0
    assert (st['trk_first'][:, :n_active[-1]] >= 0).any() and (st['trk_frames'][S - 1, n_active[-1]:] == 0).all()


def test_option_validation():
    from piml_amd.trackstats import check_options, track_stats
    assert check_options() is None and check_options(frames=(2, 9), T=9) == (2, 9)
    for bad in (dict(dt=0.0), dict(dt=float('nan')), dict(v_min=-1.0), dict(v_min=float('inf')), dict(d_max=0.0),
                dict(d_max=1025.0), dict(acc_bin=0.0), dict(acc_bin=True), dict(n_lags=0), dict(n_lags=513), dict(n_lags=1.5),
                dict(acc_bins=0), dict(acc_bins=257), dict(speed_bin=0.0), dict(speed_bins=0), dict(dur_bin=-1.0),
                dict(dur_bins=0), dict(straight_bins=0), dict(frames=(3, 3)), dict(frames=(-1, 2)), dict(frames=(0, 10), T=9),
                dict(N=65537, T=4), dict(N=65536, T=1 << 20, d_max=1024.0), dict(N=65536, T=1 << 12, acc_bin=1e4, acc_bins=256)):
        with pytest.raises(ValueError):
            check_options(**bad)
    with pytest.raises(ValueError):
        check_options(N=1, T=(1 << 25) + 1)
    assert check_options(N=65536, T=127, d_max=1024.0) is None          # 2^40 2^16 127 < 2^63
    with pytest.raises(ValueError):
        check_options(N=65536, T=128, d_max=1024.0)
    for P, M in ((np.zeros((3, 4, 3)), np.zeros((3, 4))), (np.zeros((3, 4, 2)), np.zeros((3, 5))),
                 (np.zeros((0, 4, 2)), np.zeros((0, 4)))):
        with pytest.raises(ValueError):
            track_stats(P, M)


def _synthetic():
    from piml_amd.trackstats import TrackStats, track_histograms
    rng = np.random.default_rng(0)
    S, NL, AB, N, Tp = 3, 100, 8, 30, 50
    dt = 0.1
    tau = np.arange(1, NL + 1) * float(np.float32(dt))
    n = rng.integers(60, 200, (S, NL))
    A = np.exp(-tau / 2.0)                                        # persistence time 2 s
    msd = 1.7 * tau ** 2                                          # ballistic
    arrays = dict(ac_n=n, ac_sum=np.rint(n * A * Q).astype(np.int64), msd_n=n, msd_sum=np.rint(n * msd * Q).astype(np.int64),
                  msd_far=rng.integers(0, 3, (S, NL)), acc=rng.integers(1, 50, (S, AB + 1)))
    arrays['acc_sum'] = arrays['acc'][:, :-1].sum(1) * (3 * Q // 4)
    frames = rng.integers(2, Tp + 1, (S, N))
    first = rng.integers(0, 3, (S, N))
    first = np.minimum(first, Tp - frames)
    path = rng.integers(Q // 2, 4 * Q, (S, N))
    arrays.update(trk_frames=frames, trk_steps=frames - 1, trk_first=first, trk_last=first + frames - 1, trk_path=path,
                  trk_net=(path * rng.random((S, N))).astype(np.int64))
    opts = dict(dt=dt, v_min=0.1, n_lags=NL, d_max=64.0, acc_bin=0.5, acc_bins=AB, speed_bin=0.1, speed_bins=40, dur_bin=1.0,
                dur_bins=6, straight_bins=10, frames=(0, Tp))
    arrays.update(track_histograms(arrays, Tp, dt, 0.1, 40, 1.0, 6, 10))
    return TrackStats(arrays, opts), arrays, opts


def test_host_histograms_complete_against_all():
    from piml_amd.trackstats import track_histograms
    Tp, dt = 50, 0.08
    rows = dict(trk_frames=[[50, 10, 10, 1, 0, 30]], trk_steps=[[49, 9, 9, 0, 0, 20]], trk_first=[[0, 5, 0, 7, -1, 10]],
                trk_last=[[49, 14, 9, 7, -1, 48]], trk_path=[[49 * Q // 10, 9 * Q // 10, 0, 0, 0, 2 * Q]],
                trk_net=[[49 * Q // 10, Q // 2, 0, 0, 0, 2 * Q + 3]])
    h = track_histograms(rows, Tp, dt, speed_bin=0.5, speed_bins=4, dur_bin=1.0, dur_bins=3, straight_bins=4)
    # tracks with a step: 0, 1, 2, 5; complete (first > 0 and last < 49): 1 and 5
    assert h['dur_hist'][0].tolist() == [[2, 0, 2], [1, 0, 1]]            # 4.0, 0.8, 0.8, 2.4 s, clipped into the last bin
    # mean speeds 0.1 / 0.08 = 1.25, 1.25, 0, 2 / (20 x 0.08) = 1.25 m/s
    assert h['speed_hist'][0].tolist() == [[1, 0, 3, 0], [0, 0, 2, 0]]
    # straightness 1, 5 / 9, (left out: no path), just above 1 -> the last bin
    assert h['straight_hist'][0].tolist() == [[0, 0, 1, 2], [0, 0, 1, 1]] and h['straight_n'][0].tolist() == [3, 2]
    assert h['straight_sum'][0, 1] == (Q // 2 * Q + (9 * Q // 10) // 2) // (9 * Q // 10) + Q          # clipped at 1


def test_derived_quantities_pooling_json_and_compare(tmp_path):
    from piml_amd.trackstats import ADDITIVE, TrackStats, compare_track_stats, merge
    st, arrays, opts = _synthetic()
    assert st.members == 3 and st.pooled().members == 1 and st.member(1).ac_n.shape == (1, 100)
    assert np.array_equal(st.pooled().ac_sum[0], arrays['ac_sum'].sum(0)) and st.pooled().trk_frames is None
    assert np.array_equal(st.select([2, 0]).trk_path, arrays['trk_path'][[2, 0]])
    assert np.array_equal(st.select([2, 0]).pooled().acc[0], arrays['acc'][2] + arrays['acc'][0])
    with pytest.raises(IndexError):
        st.select([3])
    tau = st.lag_times
    assert tau[0] == pytest.approx(0.1) and tau[-1] == pytest.approx(10.0)
    assert st.heading_autocorrelation() == pytest.approx(np.exp(-tau / 2.0), abs=1e-5)
    assert np.isnan(st.heading_autocorrelation(min_count=10 ** 6)).all() and math.isnan(st.persistence_time(10 ** 6))
    # exp(-tau / 2) crosses 1 / e at 2 s; the chord between 2.0 and 2.1 s (the first lag below) meets it within 1e-3
    assert st.persistence_time() == pytest.approx(2.0, abs=2e-3)
    assert st.msd() == pytest.approx(1.7 * tau ** 2, rel=1e-5)
    assert st.msd_exponent() == pytest.approx(2.0, abs=1e-4)
    diffusive = TrackStats({**arrays, 'msd_sum': np.rint(arrays['msd_n'] * 0.9 * tau * Q).astype(np.int64)}, opts)
    assert diffusive.msd_exponent() == pytest.approx(1.0, abs=1e-4)
    assert math.isnan(st.msd_exponent(tau_range=(0.5, 0.55))) and math.isnan(st.msd_exponent(min_count=10 ** 6))
    never = TrackStats({**arrays, 'ac_sum': arrays['ac_n'] * (Q // 2)}, opts)
    assert math.isnan(never.persistence_time())
    at_once = TrackStats({**arrays, 'ac_sum': arrays['ac_n'] * (Q // 4)}, opts)
    assert at_once.persistence_time() == pytest.approx(0.1)
    d = st.acceleration_density()
    assert d.shape == (9,) and d.sum() == pytest.approx(1.0) and d[3] == pytest.approx(arrays['acc'][:, 3].sum() / arrays['acc'].sum())
    assert st.mean_acceleration() == pytest.approx(0.75, abs=1e-6)
    for f in (st.duration_density, st.speed_density, st.straightness_density):
        assert f().sum() == pytest.approx(1.0) and f('complete').sum() == pytest.approx(1.0)
        with pytest.raises(ValueError):
            f('some')
    n_all, n_complete = int(st.pooled().dur_hist[0, 0].sum()), int(st.pooled().dur_hist[0, 1].sum())
    assert n_all == 90 and 0 < n_complete < n_all
    ratio = (arrays['trk_net'] / arrays['trk_path']).mean()
    assert st.mean_straightness() == pytest.approx(ratio, abs=1e-6) and 0 < st.mean_straightness('complete') < 1
    # JSON
    back = TrackStats.from_json(st.to_json(str(tmp_path / 't.json')))
    again = TrackStats.from_json(str(tmp_path / 't.json'))
    for k in ADDITIVE + ('trk_path', 'trk_first'):
        assert np.array_equal(getattr(back, k), getattr(st, k)) and np.array_equal(getattr(again, k), getattr(st, k)), k
    assert back.options == st.options
    with pytest.raises(ValueError):
        TrackStats.from_json({'version': 99})
    pooled = TrackStats.from_json(st.pooled().to_json())
    assert pooled.trk_path is None and np.array_equal(pooled.msd_sum, st.pooled().msd_sum)
    assert st.to_json()['pooled']['persistence_time'] == pytest.approx(2.0, abs=2e-3)
    # compare
    c = compare_track_stats(st, back)
    assert set(c) == {'heading_ac_max_diff', 'heading_ac_bins', 'persistence_time_diff', 'msd_exponent_diff', 'acc_l1',
                      'mean_acceleration_diff', 'straightness_l1', 'speed_l1', 'duration_l1'}
    assert c['heading_ac_bins'] == 100 and all(v == 0 for k, v in c.items() if k != 'heading_ac_bins')
    c2 = compare_track_stats(st, diffusive)
    assert c2['msd_exponent_diff'] == pytest.approx(1.0, abs=2e-4) and c2['heading_ac_max_diff'] == 0
    c3 = compare_track_stats(st.member(0), st.member(1), min_count=1)
    assert 0 < c3['acc_l1'] <= 2 and 0 < c3['straightness_l1'] <= 2 and 0 < c3['duration_l1'] <= 2 and c3['speed_l1'] > 0
    assert math.isnan(compare_track_stats(st, st, min_count=10 ** 6)['heading_ac_max_diff'])
    for k, v in (('dt', 0.08), ('v_min', 0.2), ('n_lags', 64), ('d_max', 3.0), ('acc_bin', 0.25), ('acc_bins', 9),
                 ('speed_bin', 0.2), ('speed_bins', 20), ('dur_bin', 2.0), ('dur_bins', 7), ('straight_bins', 5)):
        with pytest.raises(ValueError):
            compare_track_stats(st, TrackStats(arrays, {**opts, k: v}))
    # merge: added in list order, no track rows
    mg = merge([st, st.member(0)])
    assert mg.members == 1 and mg.trk_frames is None and mg.options['frames'] == (0, 50)
    assert np.array_equal(mg.msd_n[0], arrays['msd_n'].sum(0) + arrays['msd_n'][0])
    assert np.array_equal(mg.dur_hist[0], st.pooled().dur_hist[0] + st.dur_hist[0])
    assert merge([st, TrackStats(arrays, {**opts, 'frames': (1, 51)})]).options['frames'] is None
    assert TrackStats.merge([st]).acc_sum.tolist() == [int(arrays['acc_sum'].sum())]
    with pytest.raises(ValueError):
        merge([st, TrackStats(arrays, {**opts, 'd_max': 4.0})])
    with pytest.raises(ValueError):
        merge([])


def test_cli_parsing():
    from piml_amd import simulate, trackstats
    a = trackstats.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'r.npy', '--frames', '3:400', '--lags', '64', '--out', 'o.json'])
    assert a.data == ['a.npy', 'b.npy'] and a.ref == 'r.npy' and a.frames == (3, 400) and a.lags == 64 and a.out == 'o.json'
    d = trackstats.get_args(['--data', 'a.npy'])
    assert d.lags == 128 and d.frames is None and d.dt is None and d.d_max == 64.0 and d.acc_bins == 40 and d.v_min == 0.1
    for bad in (['--data', 'a.npy', '--lags', '0'], ['--data', 'a.npy', '--lags', '513'], ['--data', 'a.npy', '--frames', '5:5'],
                ['--data', 'a.npy', '--d_max', '2000'], ['--data', 'a.npy', '--dt', '0'], ['--lags', '4']):
        with pytest.raises(SystemExit):
            trackstats.get_args(bad)
    own, _ = simulate.get_args(['--seeds', '0:2', '--track-stats', 't.json', '--frames', '40'])
    assert own.track_stats == 't.json' and own.stats is None and own.pair_stats is None and own.flow_stats is None
    assert simulate._stats_path(own) == 't.json'
    own, _ = simulate.get_args(['--frames', '40'])
    assert own.track_stats is None and simulate._stats_path(own) == ''
    own, _ = simulate.get_args(['--law', 'mlapm', '--seeds', '0:2', '--track-stats', 't.json', '--flow-stats', 'f.json'])
    assert simulate._stats_path(own) == 'f.json, t.json'
    st, _, _ = _synthetic()
    buf = io.StringIO()
    trackstats.print_track_stats(st, 'synthetic', file=buf)
    text = buf.getvalue()
    assert 'persistence time 2.0' in text and 'MSD exponent 2.000' in text and 'tau   0.10 s' in text


def test_library_exports_constants_and_rejects_bad_arguments():
    from test_abi import declared_symbols
    from piml_amd import _lib, ops_metrics
    names = {'piml_track_stats', 'piml_track_stats_workspace_bytes'}
    assert names <= set(declared_symbols()) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    header = open(os.path.join(REPO, 'include', 'piml_hip.h')).read()
    defined = {k: int(v) for k, v in re.findall(r'#define (PIML_TRACK_[A-Z_]+) (\d+)', header)}
    assert defined == {'PIML_TRACK_TILE': ops_metrics.TRACK_TILE, 'PIML_TRACK_LAG_LANES': ops_metrics.TRACK_LAG_LANES,
                       'PIML_TRACK_MAX_LAGS': ops_metrics.TRACK_MAX_LAGS}
    assert ops_metrics.TRACK_MAX_N == 65536 and ops_metrics.TRACK_Q == Q
    fake = 1 << 20          # never dereferenced: every call below returns before any HIP call
    inf, nan = float('inf'), float('nan')

    def call(S=1, T=4, N=3, t0=0, t1=4, dt=0.08, vm=0.1, NL=4, dmax=64.0, ab=0.25, AB=40, nul=fake, out=fake, ws=fake,
             wsb=1 << 20):
        return L.piml_track_stats(nul, fake, None, S, T, N, t0, t1, dt, vm, NL, dmax, ab, AB, fake, fake, fake, out, fake,
                                  fake, fake, fake, fake, fake, fake, fake, out, ws, wsb, None)
    for bad in (dict(S=-1), dict(T=-1, t1=-1), dict(N=-1), dict(N=65537), dict(t0=-1), dict(t1=5), dict(t0=3, t1=2),
                dict(dt=0.0), dict(dt=-0.08), dict(dt=nan), dict(dt=inf), dict(vm=0.0), dict(vm=nan), dict(vm=inf),
                dict(dmax=0.0), dict(dmax=nan), dict(dmax=inf), dict(dmax=1024.5), dict(ab=0.0), dict(ab=nan), dict(ab=inf),
                dict(NL=0), dict(NL=513), dict(NL=-1), dict(AB=0), dict(AB=257),
                dict(N=65536, T=128, t1=128, dmax=1024.0),                      # 2^20 2^20 2^16 2^7 = 2^63
                dict(N=65536, T=4096, t1=4096, ab=1e4, AB=256), dict(ab=3e38, AB=2),
                dict(N=1, T=(1 << 25) + 1, t1=(1 << 25) + 1),                   # a track's path sum
                dict(nul=None), dict(out=None), dict(ws=None), dict(wsb=8), dict(wsb=(5 * 4 + 42) * 8 - 1)):
        assert call(**bad) == 1, bad
    assert call(N=65536, T=127, t1=127, dmax=1024.0, S=0) == 0 and call(N=1, T=1 << 25, t1=1 << 25, S=0) == 0
    # nothing to do: success, before the buffers are looked at
    for noop in (dict(S=0), dict(N=0), dict(t0=2, t1=2), dict(T=0, t1=0), dict(S=0, nul=None, ws=None, wsb=0)):
        assert call(**noop) == 0, noop
    assert L.piml_track_stats_workspace_bytes(2, 128, 40) == 2 * (5 * 128 + 42) * 8
    assert L.piml_track_stats_workspace_bytes(1, 4, 40) == (5 * 4 + 42) * 8
    assert L.piml_track_stats_workspace_bytes(0, 4, 40) == 0
    for bad in ((-1, 4, 40), (2, -1, 40), (2, 4, -1)):
        assert L.piml_track_stats_workspace_bytes(*bad) == -1


def test_new_kernels_use_no_scratch():
    from piml_amd import _lib
    use = _lib.kernel_resource_usage()
    for name in ('track_stats_kernel', 'track_stats_copy_kernel'):
        assert name in use, name
        assert use[name]['scratch_bytes'] == 0 and use[name]['vgpr_spill'] == 0, (name, use[name])
