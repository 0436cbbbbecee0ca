"""CPU: the numpy restatement of the measurement-line statistics (linestats_ref.py) against hand counts on dyadic numbers,
the host half on hand-made integer rows, the option and line checks, parse_lines / auto_lines, the LineStats container
(pooled / select / merge / JSON), the comparison and its refusals, the C entry's argument refusals (no compute call without
a GPU) and simulate's --line-stats / --lines pairing."""
import json

import numpy as np
import pytest

import linestats_ref as REF

Q = REF.Q


def _stats(P, M, lines, **kw):
    """a LineStats from the reference's float32 run and the package's host half (no device)"""
    from piml_amd import linestats as LS
    want = REF.line_stats(P, M, lines, **kw)
    o = dict(dt=0.08, v_bin=0.1, v_bins=40, w_bins=16, h_bin=0.25, h_bins=80, tt_bin=1.0, tt_bins=60, frames=None)
    o.update(kw)
    o.pop('n_active', None)
    arrays = {k: want[k] for k in REF.OUTPUTS}
    arrays.update(LS.host_rows(arrays, o['dt'], o['h_bin'], o['h_bins'], o['tt_bin'], o['tt_bins']))
    M = np.asarray(M)
    S, T = M.shape[:2] if M.ndim == 3 else (1, M.shape[0])
    o['frames'] = o['frames'] or (0, T)
    arrays['slices'] = np.full(S, o['frames'][1] - o['frames'][0], np.int64)
    rows = LS.check_lines(lines)
    o.update(lines=rows.astype(np.float64).tolist(), n_lines=int(rows.shape[0]), lines_hash=LS.lines_hash(rows))
    return LS.LineStats(arrays, o), want


def _random_case(S=3, T=30, N=40, seed=5, speed=1.0):
    """walkers on straight tracks through a 10 x 10 m square, with absences"""
    rng = np.random.default_rng(seed)
    start = rng.random((S, 1, N, 2)) * 10.0
    v = rng.normal(0.0, speed, (S, 1, N, 2))
    P = (start + v * 0.08 * np.arange(T)[None, :, None, None] * 4).astype(np.float32)
    M = (rng.random((S, T, N)) < 0.9).astype(np.float32)
    lines = np.array([[5, 0, 5, 10], [0, 5, 10, 5], [2, 2, 8, 7]], np.float32)
    return P, M, lines


def test_reference_against_hand_counts():
    from piml_amd.linestats import host_rows
    P, M, lines, kw, hand = REF.analytic_scene()
    want = REF.line_stats(P, M, lines, **kw)
    assert want['n_items'] == 127 * 4 and want['n_ambiguous'] == 0
    for k in REF.OUTPUTS + REF.HISTS:
        assert np.array_equal(want[k], hand[k]), (k, want[k], hand[k])
        assert np.array_equal(want['f64'][k], hand[k]), (k, 'float64 run')
    host = host_rows(hand, kw['dt'], kw['h_bin'], kw['h_bins'], kw['tt_bin'], kw['tt_bins'])
    for k in REF.HISTS:
        assert np.array_equal(host[k], hand[k]), k
    assert np.array_equal(hand['cross'].sum(-1), hand['trk_count'].sum(-1)) and (hand['nt'][..., -1] == 0).all()
    assert np.array_equal(hand['nt'].sum(-1), hand['cross']) and np.array_equal(hand['speed'].sum(-1), hand['cross'])


def test_reference_single_walkers_and_derived_quantities():
    """each special walker of the analytic scene alone, and the derived quantities of the whole"""
    P, M, lines, kw, hand = REF.analytic_scene()
    one = lambda n: REF.line_stats(P[:, :, n:n + 1], M[:, :, n:n + 1], lines, **kw)
    turn, on_line, ends_on, corner, absent, still = (one(n) for n in (REF.D, REF.E, REF.F, REF.G, REF.H, REF.I))
    assert turn['trk_count'][0, 0, 0] == 3 and turn['trk_first'][0, 0, 0] == 3 * Q // 2 and turn['trk_dir'][0, 0, 0] == 1
    assert turn['cross'][0, 0].tolist() == [1, 2]
    assert on_line['cross'][0].sum() == 1 and on_line['trk_first'][0, 0, 0] == 2 * Q and on_line['trk_dir'][0, 0, 0] == 1
    assert ends_on['cross'][0].sum() == 1 and ends_on['trk_first'][0, 0, 0] == Q and ends_on['trk_dir'][0, 0, 0] == 0
    assert corner['cross'][0, 0].sum() == 0 and corner['cross'][0, 3].tolist() == [0, 1] and corner['profile'][0, 3, 1, 0] == 1
    assert absent['cross'].sum() == 0 and absent['steps'][0] == 11
    assert still['cross'].sum() == 0 and still['steps'][0] == 13
    st, _ = _stats(P, M, lines, **kw)
    assert np.array_equal(st.flow(), hand['cross'][0] / 7.0)                # 14 frames of 0.5 s
    assert np.array_equal(st.specific_flow()[:2], st.flow()[:2] / 4.0) and st.specific_flow()[2, 0] == 1 / 7.0 / 8.0
    assert np.array_equal(st.n_t()[0, 1], np.cumsum(hand['nt'][0, 0, 1]))
    assert st.n_t()[0, :, -1].tolist() == [3, 5]
    assert st.flow_series(2.0).shape == (4, 2, 3) and st.flow_series(2.0)[0, 1].tolist() == [2.0, 0.5, 0.0]
    assert st.mean_crossing_speed()[0].tolist() == [2.75 / 3, 5.75 / 5] and np.isnan(st.mean_crossing_speed()[1, 0])
    assert st.crossing_speed_density()[0, 1, 2] == 4 / 5 / 0.5 and st.profile_density()[0, 1].tolist() == [1.6, 0.8, 0.0, 1.6]
    assert st.mean_headway()[0].tolist() == [1.75, 2.0 / 3] and st.mean_headway()[1, 1] == 1.5
    assert st.headway_density()[0, 1, :2].tolist() == [2 / 3, 1 / 3]
    assert st.mean_travel_time()[0, 1] == 3.5 and np.isnan(st.mean_travel_time()[1, 0])
    assert st.travel_time_density(0, 1)[3] == 1.0 and st.od_counts()[0].tolist() == [0, 2, 0, 0]
    assert st.od_fraction()[0, 1] == 1.0 and np.isnan(st.od_fraction()[1]).all()


def test_reference_participation_window_and_bounds():
    P, M, lines, kw, hand = REF.analytic_scene()
    P2, M2 = P.copy(), M.copy()
    M2[0, 2, REF.A], P2[0, 3, REF.A, 0], P2[0, 5, REF.B, 1], P2[0, 4, REF.C, 0] = 0.5, 65536.0, np.nan, -np.inf
    w = REF.line_stats(P2, M2, lines, **kw)
    assert w['cross'][0, 0].tolist() == [2, 3] and w['n_ambiguous'] == 0    # A's, B's and C's crossings of line 0 are gone
    win = REF.line_stats(P, M, lines, frames=(2, 7), **kw)
    assert win['nt'].shape[-1] == 5 and win['cross'][0, 0].tolist() == [2, 4] and win['trk_first'][0, 0, REF.A] == Q // 2
    few = REF.line_stats(P, M, lines, n_active=[4], **kw)
    assert few['cross'][0, 0].tolist() == [2, 4] and (few['trk_first'][0, :, 4:] == -1).all() and few['tracks'][0] == 4
    none = REF.line_stats(P[:, :1], M[:, :1], lines, **kw)
    assert none['steps'][0] == 0 and none['n_items'] == 0 and (none['trk_dir'] == -1).all() and none['nt'].shape[-1] == 1


def test_reference_ambiguity_on_random_tracks():
    P, M, lines = _random_case(S=2, T=40, N=300)
    want = REF.line_stats(P, M, lines)
    print(f'\n[linestats] {want["n_items"]} items, {want["n_ambiguous"]} ambiguous')
    assert want['n_items'] > 40000 and want['n_ambiguous'] / want['n_items'] <= 1e-3
    assert want['cross'].sum() > 100 and want['travel_n'].sum() > 0 and want['headway_n'].sum() > 0


def test_host_rows_from_hand_made_rows():
    from piml_amd.linestats import host_rows
    # two lines, six tracks: ties in trk_first (tracks 0 and 1 on line 0), tracks with one line only (2: line 0, 3: line 1), one
    # that crosses line 1 first (4) and one without a crossing or a step (5)
    first = np.array([[[4 * Q, 4 * Q, 6 * Q, -1, 9 * Q, -1], [8 * Q, 4 * Q + 1, -1, 2 * Q, 3 * Q, -1]]])
    dirs = np.array([[[0, 0, 0, -1, 1, -1], [1, 1, -1, 1, 0, -1]]])
    rows = dict(trk_steps=np.array([[5, 5, 2, 1, 7, 0]]), trk_first=first, trk_dir=dirs)
    kw = dict(dt=0.5, h_bin=0.5, h_bins=3, tt_bin=1.0, tt_bins=2)
    h = host_rows(rows, **kw)
    mine = REF.host_rows(rows, **kw)
    for k in REF.HISTS:
        assert np.array_equal(h[k], mine[k]), k
    assert h['tracks'].tolist() == [5]
    assert h['headway'][0, 0, 0].tolist() == [1, 0, 1, 0]                  # 4 Q, 4 Q, 6 Q: a tie (0 s) and 2 frames (1 s)
    assert h['headway'][0, 1, 1].tolist() == [0, 0, 1, 1] and h['headway_sum'][0, 1, 1] == 6 * Q   # 2 Q, 4 Q + 1, 8 Q
    assert h['headway_n'][0].tolist() == [[2, 0], [0, 2]]
    assert h['travel_n'][0].tolist() == [[0, 2], [1, 0]]                   # 0 -> 1: tracks 0 (2 s) and 1 (one unit: 0 s)
    assert h['travel'][0, 0, 1].tolist() == [1, 0, 1] and h['travel'][0, 1, 0].tolist() == [0, 0, 1]   # 4: 6 frames, open bin
    assert h['travel_sum'][0, 0, 1] == 4 * Q + 1 and h['travel_sum'][0, 1, 0] == 6 * Q
    # L = 1 and a member without crossings
    solo = dict(trk_steps=np.array([[3, 3], [4, 0]]), trk_first=np.array([[[Q, 3 * Q]], [[-1, -1]]]),
                trk_dir=np.array([[[1, 1]], [[-1, -1]]]))
    h = host_rows(solo, **kw)
    mine = REF.host_rows(solo, **kw)
    for k in REF.HISTS:
        assert np.array_equal(h[k], mine[k]), k
    assert h['travel'].shape == (2, 1, 1, 3) and h['travel'].sum() == 0 and h['headway'][0, 0, 1].tolist() == [0, 0, 1, 0]
    assert h['headway'][1].sum() == 0 and h['tracks'].tolist() == [2, 1]


def test_option_and_line_validation():
    from piml_amd.linestats import check_lines, check_options, line_stats
    assert check_options() is None and check_options(frames=(2, 5), T=5) == (2, 5)
    for kw in (dict(dt=0), dict(dt=float('nan')), dict(v_bin=-1), dict(v_bin=True), dict(h_bin=0), dict(h_bin=1e-60),
               dict(tt_bin=float('inf')), dict(v_bins=0), dict(v_bins=257), dict(w_bins=0), dict(w_bins=257), dict(h_bins=0),
               dict(h_bins=257), dict(tt_bins=1.5), dict(tt_bins=0), dict(tt_bins=257), dict(frames=(3, 3)), dict(frames=(-1, 2)),
               dict(frames=(0, 9), T=8), dict(N=65537, T=4), dict(T=(1 << 25) + 1), dict(v_bin=1e30, N=65536, T=1 << 20)):
        with pytest.raises(ValueError):
            check_options(**kw)
    ok = check_lines([[0, 0, 1, 0]] * 16)
    assert ok.shape == (16, 4) and ok.dtype == np.float32 and check_lines([0, 0, 0, 1]).shape == (1, 4)
    tiny = np.float64(np.float32(1.0)) + 1e-12                            # a != b in float64, equal after rounding
    for bad in ([], np.zeros((0, 4)), [[0, 0, 1, 0]] * 17, [[1, 2, 1, 2]], [[1.0, 2.0, tiny, 2.0]], [[0, 0, np.nan, 1]],
                [[0, np.inf, 0, 1]], [[0, 0, 65536.0, 1]], [[0, 0, 1]], [[0, 0, 1e39, 1]], 'nonsense'):
        with pytest.raises(ValueError):
            check_lines(bad)
    # refused on the host before anything touches a device
    P, M = np.zeros((2, 3, 2), np.float32), np.ones((2, 3), np.float32)
    for lines, kw in (([[1, 1, 1, 1]], {}), ([[0, 0, 1, 0]], dict(v_bins=0)), ([[0, 0, 1, 0]], dict(frames=(0, 3)))):
        with pytest.raises(ValueError):
            line_stats(P, M, lines, **kw)


def test_parse_lines_and_auto_lines():
    from piml_amd.linestats import auto_lines, lines_hash, parse_lines
    assert parse_lines('auto') == 'auto'
    got = parse_lines('0,15,30,15; 15,0,15,30.5;')
    assert got.dtype == np.float32 and got.tolist() == [[0, 15, 30, 15], [15, 0, 15, 30.5]]
    for bad in ('', ';', '1,2,3', '1,2,3,4,5', 'a,b,c,d', '1,1,1,1', ';'.join(['0,0,1,0'] * 17), '0,0,nan,1'):
        with pytest.raises(ValueError):
            parse_lines(bad)
    two = auto_lines((0.0, 30.0, -4.0, 16.0))
    assert two.tolist() == [[15, -4, 15, 16], [0, 6, 30, 6]]                # bottom to top, then left to right
    for bad in ((0, 0, 0, 1), (0, 1, 2, 1), (0, float('nan'), 0, 1)):
        with pytest.raises(ValueError):
            auto_lines(bad)
    assert lines_hash(two) == lines_hash(two.astype(np.float64).tolist()) != lines_hash(two[::-1])


def test_container_pooled_select_merge_json(tmp_path):
    from piml_amd import linestats as LS
    P, M, lines = _random_case()
    st, want = _stats(P, M, lines, h_bin=0.5)
    assert st.members == 3 and st.n_lines == 3 and st.cross.sum() > 50 and st.trk_first.shape == (3, 3, 40)
    assert st.headway_n.sum() > 0 and st.travel_n.sum() > 0
    pool = st.pooled()
    assert pool.members == 1 and pool.trk_first is None and pool.slices[0] == 90
    for k in LS.ADDITIVE:
        assert np.array_equal(getattr(pool, k)[0], getattr(st, k).sum(0)), k
    sel = st.select([2, 0, 0])
    assert sel.members == 3 and np.array_equal(sel.nt[1], st.nt[0]) and np.array_equal(sel.trk_first[0], st.trk_first[2])
    assert np.array_equal(st.member(1).speed, st.speed[1:2])
    with pytest.raises(IndexError):
        st.select([3])
    # additivity: pooling two members equals adding them, the host histograms included
    pair = st.select([0, 2]).pooled()
    for k in LS.ADDITIVE:
        assert np.array_equal(getattr(pair, k)[0], getattr(st.member(0), k)[0] + getattr(st.member(2), k)[0]), k
    merged = LS.merge([st.member(0), st.member(1), st.member(2)])
    for k in LS.ADDITIVE:
        assert np.array_equal(getattr(merged, k), getattr(pool, k)), k
    assert LS.LineStats.merge([st, st]).cross.sum() == 2 * pool.cross.sum()
    assert np.array_equal(st.flow(), pool.cross[0] / (90 * float(np.float32(0.08))))
    short, _ = _stats(P[:1, :20], M[:1, :20], lines, h_bin=0.5)
    mixed = LS.merge([st, short])
    assert mixed.nt is None and mixed.options['frames'] is None and mixed.slices[0] == 110
    with pytest.raises(ValueError):
        mixed.n_t()
    assert np.isfinite(mixed.flow()).all()
    path = str(tmp_path / 'lines.json')
    d = st.to_json(path)
    back = LS.LineStats.from_json(path)
    assert back.options == st.options
    for k in LS.ARRAYS:
        assert np.array_equal(getattr(back, k), getattr(st, k)), k
    assert json.dumps(back.to_json()) == json.dumps(d)
    assert LS.LineStats.from_json(pool.to_json()).trk_count is None and LS.LineStats.from_json(mixed.to_json()).nt is None
    with pytest.raises(ValueError):
        LS.LineStats.from_json({**d, 'version': 99})
    with pytest.raises(ValueError):
        LS.merge([])
    assert d['pooled']['cross'] == pool.cross[0].tolist() and d['pooled']['tracks'] == int(st.tracks.sum())


def test_compare_line_stats_and_its_refusals():
    from piml_amd import linestats as LS
    P, M, lines, kw, hand = REF.analytic_scene()
    a, _ = _stats(P, M, lines, **kw)
    # b: the same scene with walker B gone and walker C walking at A's pace
    P2, M2 = P.copy(), M.copy()
    M2[0, :, REF.B] = 0
    P2[0, :, REF.C, 0] = 2.3125 - 0.625 * (np.arange(14) - 4)
    b, _ = _stats(P2, M2, lines, **kw)
    assert b.cross[0, 0].tolist() == [3, 4] and b.cross[0, 1].tolist() == [0, 1]
    c = LS.compare_line_stats(a, b, min_count=3)
    assert set(c) >= {'flow_rel_diff', 'direction_split_diff', 'speed_l1', 'profile_l1', 'headway_l1', 'travel_l1',
                      'mean_travel_rel_diff'}
    # entries with >= 3 crossings on the b side: line 0 backwards (3 vs 3) and forwards (5 vs 4)
    assert c['flow_rel_diff'] == pytest.approx((0 + 0.25) / 2) and c['direction_split_diff'] == pytest.approx(abs(3 / 8 - 3 / 7))
    # speed shares: backwards a (0, 2/3, 1/3) b (0, 1/3, 2/3); forwards a (0, .2, .8) b (0, .25, .75); profile shares:
    # backwards equal, forwards a (.4, .2, 0, .4) b (.5, 0, 0, .5)
    assert c['speed_l1'] == pytest.approx((2 / 3 + 0.1) / 2) and c['profile_l1'] == pytest.approx((0 + 0.4) / 2)
    assert np.isnan(c['travel_l1']) and np.isnan(c['mean_travel_rel_diff']) and np.isnan(c['headway_l1'])
    low = LS.compare_line_stats(a, b, min_count=1)
    assert low['travel_l1'] == 0.0 and low['mean_travel_rel_diff'] == 0.0 and low['headway_l1'] > 0
    same = LS.compare_line_stats(a, a, min_count=1)
    assert all(v == 0 for v in same.values())
    assert all(np.isnan(v) for v in LS.compare_line_stats(a, b, min_count=50).values())
    other, _ = _stats(P, M, lines, **{**kw, 'h_bin': 2.0})
    with pytest.raises(ValueError, match='options'):
        LS.compare_line_stats(a, other)
    slow, _ = _stats(P, M, lines, **{**kw, 'dt': 0.25})
    with pytest.raises(ValueError, match='options'):
        LS.compare_line_stats(a, slow)
    moved = lines.copy()
    moved[1, 0] = np.nextafter(moved[1, 0], np.float32(np.inf))
    for changed in (moved, lines[:3]):
        d, _ = _stats(P, M, changed, **kw)
        with pytest.raises(ValueError, match='lines'):
            LS.compare_line_stats(a, d)
        with pytest.raises(ValueError):
            LS.merge([a, d])


def _call(L, S=1, T=4, N=8, t0=0, t1=4, n_lines=2, dt=0.08, v_bin=0.1, v_bins=40, w_bins=16):
    return L.piml_line_stats(None, None, None, S, T, N, t0, t1, None, n_lines, dt, v_bin, v_bins, w_bins, *([None] * 10), None, 0,
                             None)


def test_entry_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib, ops_metrics
    assert _lib.ABI_VERSION == 35
    L = _lib.lib()
    assert (ops_metrics.LINE_MAX_L, ops_metrics.LINE_MAX_N, ops_metrics.LINE_MAX_BINS, ops_metrics.LINE_Q) == (16, 65536, 256, Q)
    inf, nan = float('inf'), float('nan')
    for kw in (dict(S=-1), dict(T=-1, t1=0), dict(N=-1), dict(N=65537), dict(n_lines=-1), dict(n_lines=17), dict(t0=-1),
               dict(t1=5), dict(t0=3, t1=2), dict(dt=0.0), dict(dt=nan), dict(dt=inf), dict(v_bin=0.0), dict(v_bin=nan),
               dict(v_bin=-1.0), dict(v_bins=0), dict(v_bins=257), dict(w_bins=0), dict(w_bins=257),
               dict(T=(1 << 25) + 1, t1=(1 << 25) + 1),                                # the window's length
               dict(v_bin=1e30, N=65536, T=1 << 20, t1=1 << 20)):                      # v_bin v_bins Q N T' >= 2^63
        assert _call(L, **kw) == 1, kw
    # a NULL pointer where there is work to do, and empty problems
    assert _call(L) == 1
    for kw in (dict(S=0), dict(t0=2, t1=2), dict(N=0), dict(n_lines=0), dict(T=0, t1=0)):
        assert _call(L, **kw) == 0, kw
    assert L.piml_line_stats_workspace_bytes(2, 10, 3, 7, 40, 16) == 2 * (2 * 3 * (7 + 40 + 16 + 3) + 1 + 10 + 2 * 3 * 10) * 8
    assert L.piml_line_stats_workspace_bytes(1, 1, -1, 1, 1, 1) == -1


def test_line_stats_frames_refuses_cpu_tensors():
    import torch
    from piml_amd import _lib, ops_metrics
    P, M, lines = torch.zeros(1, 3, 4, 2), torch.ones(1, 3, 4), torch.tensor([[0.0, 0.0, 1.0, 0.0]])
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.line_stats_frames(P, M, lines, 0.08)


def test_simulate_line_stats_needs_lines(capsys):
    from piml_amd import simulate
    for argv in (['--line-stats', 'out.json'], ['--lines', '0,0,1,0'], ['--line-stats', 'out.json', '--lines', 'auto'],
                 ['--line-stats', 'out.json', '--lines', '1,1,1,1']):
        with pytest.raises(SystemExit) as ex:
            simulate.get_args(argv)
        assert ex.value.code == 2, argv
    assert '--line-stats' in capsys.readouterr().err
    own, _ = simulate.get_args(['--line-stats', 'out.json', '--lines', '0,15,30,15;15,0,15,30'])
    assert own.lines.shape == (2, 4) and own.line_stats == 'out.json' and simulate._stats_path(own) == 'out.json'
