"""CPU: the numpy restatement of the obstacle statistics (obstaclestats_ref.py) against hand counts on dyadic numbers, the
option checks, the ObstacleStats container (pooled / select / merge / JSON), the comparison's refusals, obstacle_spacing,
the host histograms from hand-made track rows, and the C entry's argument refusals (no compute call without a GPU)."""
import json
import warnings

import numpy as np
import pytest

import obstaclestats_ref as REF

Q = REF.Q
CAP = 1e-3                                    # the ambiguous share of items, as the sibling tests


def _stats(P, V, M, obs, **kw):
    """an ObstacleStats from the reference's float32 run and the package's host half (no device)"""
    from piml_amd import obstaclestats as OS
    want = REF.obstacle_stats(P, V, M, obs, **kw)
    arrays = {k: want[k] for k in REF.OUTPUTS}
    o = dict(dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.05, r_bins=100, tau_bin=0.1, tau_bins=100, box=None, frames=None)
    o.update(kw)
    arrays.update(OS.track_histograms(arrays, o['r_bin'], o['r_bins']))
    S, T = np.asarray(M).shape[:2] if np.asarray(M).ndim == 3 else (1, np.asarray(M).shape[0])
    o.update(frames=o['frames'] or (0, T), n_obstacles=int(np.asarray(obs).reshape(-1, 2).shape[0]),
             obstacles_hash=OS.obstacles_hash(obs))
    o.pop('n_active', None)
    return OS.ObstacleStats(arrays, o), want


def _random_case(S=3, T=6, N=40, seed=5):
    rng = np.random.default_rng(seed)
    P = (rng.random((S, T, N, 2)) * [20.0, 15.0]).astype(np.float32)
    V = rng.normal(0.0, 1.0, (S, T, N, 2)).astype(np.float32)
    M = (rng.random((S, T, N)) < 0.85).astype(np.float32)
    obs = np.concatenate([np.stack([np.arange(200) * 0.05 + 3.0, np.full(200, 7.0)], -1),
                          [[10 + np.cos(a), 4 + np.sin(a)] for a in np.linspace(0, 2 * np.pi, 50, endpoint=False)]])
    return P, V, M, obs.astype(np.float32)


def test_reference_against_hand_counts():
    from piml_amd.obstaclestats import track_histograms
    P, V, M, obs, kw, hand = REF.analytic_scene()
    want = REF.obstacle_stats(P, V, M, obs, **kw)
    assert want['n_items'] == 10 and want['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(want[k], hand[k]), (k, want[k], hand[k])
        assert np.array_equal(want['f64'][k], hand[k]), (k, 'float64 run')
    host = track_histograms(want, kw['r_bin'], kw['r_bins'])
    mine = REF.host_rows(want, kw['r_bin'], kw['r_bins'])
    for k in REF.HISTS:
        assert np.array_equal(host[k], hand[k]) and np.array_equal(mine[k], hand[k]), k


def test_reference_single_cases():
    """each agent of the analytic scene alone, and the derived quantities of the whole"""
    P, V, M, obs, kw, hand = REF.analytic_scene()
    one = lambda n: REF.obstacle_stats(P[:, :, n:n + 1], V[:, :, n:n + 1], M[:, :, n:n + 1], obs, **kw)
    tunnel, parallel, head_on, standing, away = (one(n) for n in range(5))
    assert tunnel['hit'][0] == 1 and tunnel['contact'][0] == 0 and tunnel['swept'][0, 0] == 1
    assert parallel['clear'][0, int(0.5 / kw['r_bin'])] == 2 and parallel['hit'][0] == 0 and parallel['min_ttc'][0, 16] == 2
    assert head_on['min_ttc'][0, 4] == 1 and head_on['min_ttc'][0, 3] == 1             # tau_min = 1.0, then 0.875
    assert standing['min_ttc'][0, 16] == 2 and standing['swept'][0, 6] == 1 and standing['clear_speed'].sum() == 0
    assert away['min_ttc'][0, 16] == 2 and away['hit'][0] == 0
    st, _ = _stats(P, V, M, obs, **kw)
    assert st.hit_rate() == 0.2 and st.contact_rate() == 0.0 and st.hit_track_fraction() == 0.2
    assert st.contact_track_fraction() == 0.0 and st.mean_clearance() == 0.7
    assert st.clearance_density()[4] == 0.5 / 0.125 and st.min_ttc_density()[0] == 0.1 / 0.25
    assert st.track_min_clearance_density()[4] == 0.6 / 0.125
    sp = st.speed_by_clearance(min_count=1)
    assert sp[4] == 19 / 5 and sp[6] == 0 and np.isnan(sp[0]) and np.isnan(st.speed_by_clearance(min_count=6)[4])


def test_reference_skips_invalid_points_and_counts_without_any():
    P, V, M, obs, kw, hand = REF.analytic_scene()
    bad = np.concatenate([obs, [[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan]]]).astype(np.float32)
    want = REF.obstacle_stats(P, V, M, bad[::-1], **kw)
    for k in REF.OUTPUTS:
        assert np.array_equal(want[k], hand[k]), k
    none = REF.obstacle_stats(P, V, M, bad[-3:], **kw)
    assert none['focal'][0] == 10 and none['steps'][0] == 5 and none['n_items'] == 0
    for k in REF.OUTPUTS[2:]:
        assert (none[k] == (-1 if k == 'trk_min' else 0)).all(), k
    empty = REF.obstacle_stats(P, V, M, np.zeros((0, 2)), **kw)
    assert empty['focal'][0] == 0 and (empty['trk_min'] == -1).all()
    # participation: a mask of 0.5, a coordinate of 65536, a speed of 1024 and non-finite values take no part; the box
    P2, V2, M2 = P.copy(), V.copy(), M.copy()
    M2[0, 0, 0], P2[0, 0, 1, 0], V2[0, 0, 2, 1], P2[0, 1, 3, 1], V2[0, 1, 4, 0] = 0.5, 65536.0, -1024.0, np.nan, np.inf
    w = REF.obstacle_stats(P2, V2, M2, obs, **kw)
    assert w['focal'][0] == 5 and w['steps'][0] == 0 and w['hit'][0] == 0
    boxed = REF.obstacle_stats(P, V, M, obs, box=(-1.5, 2.5, 0.0, 2.0), **kw)
    assert boxed['focal'][0] == 5 and boxed['steps'][0] == 2 and boxed['trk_frames'][0].tolist() == [1, 2, 2, 0, 0]


def test_reference_ambiguity_on_random_steps():
    """the set-up the cap was measured on: 20 000 random agent-steps in a 20 x 15 m box, an 800-point wall at 0.05 m and a
    100-point circle, radius 0.25, hit_radius 0.125, r_bin 0.1, tau_bin 0.25"""
    rng = np.random.default_rng(0)
    n = 20000
    P = np.zeros((1, 2, n, 2), np.float32)
    P[0, 0] = rng.random((n, 2)) * [20.0, 15.0]
    V = np.repeat(rng.normal(0.0, 1.0, (1, 1, n, 2)), 2, 1).astype(np.float32)
    P[0, 1] = P[0, 0] + V[0, 0] * np.float32(0.08)
    M = np.ones((1, 2, n), np.float32)
    M[0, 1, n // 2:] = 0                                         # half of the items are steps, the others single frames
    wall = np.stack([np.arange(800) * 0.05, np.full(800, 7.5)], -1)
    ang = np.linspace(0, 2 * np.pi, 100, endpoint=False)
    obs = np.concatenate([wall, np.stack([10 + np.cos(ang), 3 + np.sin(ang)], -1)]).astype(np.float32)
    want = REF.obstacle_stats(P, V, M, obs, radius=0.25, hit_radius=0.125, r_bin=0.1, tau_bin=0.25)
    print(f'\n[obstaclestats] {want["n_items"]} items, {want["n_ambiguous"]} ambiguous')
    assert want['n_items'] == n + n // 2 and want['steps'][0] == n // 2
    assert want['n_ambiguous'] / want['n_items'] <= CAP
    assert want['hit'][0] > 0 and want['contact'][0] > 0 and want['min_ttc'][0, :-1].sum() > 0


def test_check_options_refusals():
    from piml_amd.obstaclestats import check_options
    assert check_options() == (None, None)
    assert check_options(box=(0, 1, 0, 1), frames=(2, 5), T=5) == ((0.0, 1.0, 0.0, 1.0), (2, 5))
    for kw in (dict(dt=0), dict(dt=float('nan')), dict(radius=-1), dict(radius=True), dict(hit_radius=0), dict(hit_radius=1e-60),
               dict(r_bin=float('inf')), dict(tau_bin=0), dict(r_bins=0), dict(r_bins=257), dict(tau_bins=1.5), dict(tau_bins=300),
               dict(box=(0, 0, 0, 1)), dict(box=(0, 1, 2)), dict(box=(0, float('nan'), 0, 1)), dict(frames=(3, 3)),
               dict(frames=(-1, 2)), dict(frames=(0, 9), T=8), dict(N=65537, T=4), dict(O=(1 << 24) + 1),
               dict(N=65536, T=1 << 30)):
        with pytest.raises(ValueError):
            check_options(**kw)


def test_container_pooled_select_merge_json(tmp_path):
    from piml_amd import obstaclestats as OS
    P, V, M, obs = _random_case()
    st, want = _stats(P, V, M, obs, hit_radius=0.125)
    assert st.members == 3 and st.focal.sum() > 0 and st.hit.sum() > 0 and st.trk_min.shape == (3, 40)
    pool = st.pooled()
    assert pool.members == 1 and pool.trk_min is None
    for k in OS.ADDITIVE:
        assert np.array_equal(getattr(pool, k)[0], getattr(st, k).sum(0)), k
    sel = st.select([2, 0, 0])
    assert sel.members == 3 and np.array_equal(sel.clear[1], st.clear[0]) and np.array_equal(sel.trk_min[0], st.trk_min[2])
    assert np.array_equal(st.member(1).swept, st.swept[1:2])
    with pytest.raises(IndexError):
        st.select([3])
    merged = OS.merge([st.member(0), st.member(1), st.member(2)])
    for k in OS.ADDITIVE:
        assert np.array_equal(getattr(merged, k), getattr(pool, k)), k
    assert OS.ObstacleStats.merge([st, st]).focal[0] == 2 * pool.focal[0]
    path = str(tmp_path / 'walls.json')
    d = st.to_json(path)
    back = OS.ObstacleStats.from_json(path)
    assert back.options == st.options
    for k in OS.ARRAYS:
        assert np.array_equal(getattr(back, k), getattr(st, k)), k
    assert json.dumps(back.to_json()) == json.dumps(d)
    assert OS.ObstacleStats.from_json(pool.to_json()).trk_frames is None
    with pytest.raises(ValueError):
        OS.ObstacleStats.from_json({**d, 'version': 99})
    with pytest.raises(ValueError):
        OS.merge([])
    assert d['pooled']['hits'] == int(st.hit.sum()) and d['pooled']['tracks'] == int(st.tracks.sum())


def test_compare_raises_on_options_and_obstacle_sets():
    from piml_amd import obstaclestats as OS
    P, V, M, obs = _random_case()
    a, _ = _stats(P, V, M, obs, hit_radius=0.125)
    b, _ = _stats(P[:2], V[:2] * 0.5, M[:2], obs, hit_radius=0.125)
    c = OS.compare_obstacle_stats(a, b, min_count=5)
    assert set(c) == {'clearance_l1', 'min_ttc_l1', 'track_min_clearance_l1', 'contact_rate_diff', 'hit_rate_diff',
                      'hit_track_fraction_diff', 'contact_track_fraction_diff', 'mean_clearance_diff', 'speed_max_diff',
                      'speed_bins'}
    assert c['speed_bins'] > 0 and c['speed_max_diff'] > 0 and 0 < c['min_ttc_l1'] <= 2
    same = OS.compare_obstacle_stats(a, a)
    assert same['clearance_l1'] == 0 and same['hit_rate_diff'] == 0 and same['track_min_clearance_l1'] == 0
    other, _ = _stats(P, V, M, obs, hit_radius=0.1)
    with pytest.raises(ValueError, match='options'):
        OS.compare_obstacle_stats(a, other)
    moved = obs.copy()
    moved[7, 0] = np.nextafter(moved[7, 0], np.float32(np.inf))
    for changed in (moved, obs[:-1]):
        d, _ = _stats(P, V, M, changed, hit_radius=0.125)
        with pytest.raises(ValueError, match='obstacle sets'):
            OS.compare_obstacle_stats(a, d)
        with pytest.raises(ValueError):
            OS.merge([a, d])


def test_obstacle_spacing_and_its_warning():
    from piml_amd import obstaclestats as OS
    from piml_amd.scenarios import gc_scenario
    line = np.stack([np.arange(40) * 0.25, np.zeros(40)], -1)
    assert OS.obstacle_spacing(line) == 0.25
    assert OS.obstacle_spacing(np.concatenate([line, [[np.nan, 1.0], [100.0, np.inf]]])) == 0.25
    assert OS.obstacle_spacing(np.concatenate([line, [[50.0, 50.0]]]), chunk=7) == 0.25        # the median, not the mean
    assert np.isnan(OS.obstacle_spacing(line[:1])) and np.isnan(OS.obstacle_spacing(None))
    assert OS.obstacle_spacing(gc_scenario().obstacles) == pytest.approx(0.05, abs=1e-3)
    OS._warned = False
    with pytest.warns(UserWarning, match='half the obstacle spacing'):
        OS._warn_sparse(line.astype(np.float32), OS.obstacles_hash(line), 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        OS._warn_sparse(line.astype(np.float32), OS.obstacles_hash(line), 0.1)               # once per process
        OS._warned = False
        OS._warn_sparse(line.astype(np.float32), OS.obstacles_hash(line), 0.125)             # half the spacing: fine
    OS._warned = False


def test_host_histograms_from_hand_made_rows():
    from piml_amd.obstaclestats import track_histograms
    rows = dict(trk_frames=[[3, 0, 1, 5, 2]], trk_contacts=[[0, 0, 1, 2, 0]], trk_hits=[[1, 0, 0, 3, 0]],
                trk_min=[[Q // 2, -1, Q // 8, 0, 40 * Q]])
    h = track_histograms(rows, r_bin=0.25, r_bins=8)
    assert h['trk_min_hist'].tolist() == [[2, 0, 1, 0, 0, 0, 0, 0, 1]]              # 0.125 and 0 | 0.5 | 40 m: the open bin
    assert (h['tracks'][0], h['tracks_hit'][0], h['tracks_contact'][0]) == (4, 2, 2)
    mine = REF.host_rows({k: np.asarray(v) for k, v in rows.items()}, 0.25, 8)
    for k in REF.HISTS:
        assert np.array_equal(h[k], mine[k]), k
    two = track_histograms({k: np.asarray(v * 2) for k, v in rows.items()}, r_bin=0.0625, r_bins=100)
    assert two['trk_min_hist'].shape == (2, 101) and two['trk_min_hist'][1, 8] == 1 and two['trk_min_hist'][1, 2] == 1


def _call(L, S=1, T=4, N=8, t0=0, t1=4, O=16, dt=0.08, radius=0.25, hit_radius=0.1, has_box=0, box=(0., 1., 0., 1.),
          r_bin=0.05, r_bins=100, tau_bin=0.1, tau_bins=100):
    return L.piml_obstacle_stats(None, None, None, None, S, T, N, t0, t1, None, O, dt, radius, hit_radius, has_box, *box,
                                 r_bin, r_bins, tau_bin, tau_bins, *([None] * 13), None, 0, None)


def test_entry_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib, ops_metrics
    L = _lib.lib()
    assert ops_metrics.OBS_TILE == 4096 and ops_metrics.OBS_Q == Q
    inf, nan = float('inf'), float('nan')
    for kw in (dict(S=-1), dict(T=-1, t1=0), dict(N=-1), dict(O=-1), dict(N=65537), dict(O=(1 << 24) + 1), dict(t0=-1),
               dict(t1=5), dict(t0=3, t1=2), dict(dt=0.0), dict(dt=nan), dict(radius=0.0), dict(radius=inf),
               dict(hit_radius=-0.1), dict(r_bin=0.0), dict(r_bin=nan), dict(tau_bin=inf), dict(tau_bin=-1.0), dict(r_bins=0),
               dict(r_bins=257), dict(tau_bins=0), dict(tau_bins=257), dict(has_box=1, box=(1., 1., 0., 1.)),
               dict(has_box=1, box=(0., 1., 0., nan)), dict(has_box=1, box=(0., inf, 0., 1.)),
               dict(N=65536, T=1 << 30, t1=1 << 30),                                   # 1449 Q N T' >= 2^63
               dict(r_bin=1e30, N=65536, T=1 << 20, t1=1 << 20)):                      # r_bin r_bins Q N T' >= 2^63
        assert _call(L, **kw) == 1, kw
    # a NULL pointer where there is work to do, and empty problems
    assert _call(L) == 1
    for kw in (dict(S=0), dict(t0=2, t1=2), dict(N=0), dict(O=0), dict(T=0, t1=0)):
        assert _call(L, **kw) == 0, kw
    assert L.piml_obstacle_stats_workspace_bytes(2, 10, 100, 100) == 2 * (300 + 100 + 9 + 40) * 8
    assert L.piml_obstacle_stats_workspace_bytes(-1, 1, 1, 1) == -1
