"""CPU: heading-frame pair statistics (piml_amd.viewstats) without a GPU -- option validation, JSON, pooling, selecting and
merging, the derived quantities on hand-made counts (front/back ratio, passing side, headway fit), compare_view_stats,
the view side of stats_objective, the command lines' parsing, the C entry's exports and argument checks (rejected before
any HIP call), the shapes of the GPU tests' runs, and the ambiguous share of every input the GPU tests use."""
import ctypes
import math

import numpy as np
import pytest

import viewstats_ref as REF
import viewstats_shapes as SH

HALF, GB = 4, 10
G = 2 * HALF
OPTS = dict(lags=(8, 16), v_min=0.1, cell=0.5, half=HALF, cos_same=float(REF.COS_SAME), r_max=None, corridor=0.4,
            gap_bin=0.2, gap_bins=GB, box=None, frames=(0, 100))


def make(map0=None, map_s=None, pairs0=None, pairs_s=None, focal=1000, nn=None, gap=None, speed=None, members=1, opts=None):
    """a ViewStats of `members` equal members: lag-0 map map0 (4, G, G), the scrambled counts map_s on each of the two
    lags; pairs default to the maps' sums"""
    from piml_amd.viewstats import Q, ViewStats
    map0 = np.zeros((4, G, G), np.int64) if map0 is None else np.asarray(map0, np.int64)
    map_s = map0.copy() if map_s is None else np.asarray(map_s, np.int64)
    a = dict(map=np.stack([map0, map_s, map_s])[None])
    p0 = int(map0.sum()) if pairs0 is None else pairs0
    ps = int(map_s.sum()) if pairs_s is None else pairs_s
    a['pairs'] = np.array([[p0, ps, ps]], np.int64)
    a['focal'] = np.array([[focal, focal, focal]], np.int64)
    a['nn_map'] = np.zeros((1, G * G + 1), np.int64)
    a['nn_map'][0, -1 if nn is None else nn] = focal
    a['front_gap'] = np.zeros((1, GB + 1), np.int64)
    a['front_speed'] = np.zeros((1, GB), np.int64)
    if gap is None:
        a['front_gap'][0, -1] = focal
    else:
        a['front_gap'][0, :GB] = gap
        a['front_gap'][0, GB] = focal - int(np.sum(gap))
        a['front_speed'][0] = np.round(np.asarray(speed, np.float64) * np.asarray(gap) * Q).astype(np.int64)
    a = {k: np.repeat(v, members, axis=0) for k, v in a.items()}
    return ViewStats(a, dict(OPTS if opts is None else opts))


def test_options_are_validated():
    from piml_amd.viewstats import check_options
    lags, box, frames = check_options(lags=[3, 9], box=[0, 1, 2, 3], frames=(2, 9), T=10)
    assert lags == (3, 9) and box == (0.0, 1.0, 2.0, 3.0) and frames == (2, 9)
    assert check_options(lags=())[0] == ()
    for bad in (dict(half=0), dict(half=17), dict(half=2.5), dict(gap_bins=0), dict(gap_bins=257), dict(cell=0.0),
                dict(v_min=-1.0), dict(corridor=float('nan')), dict(gap_bin=float('inf')), dict(cos_same=1.5),
                dict(cos_same=-0.1), dict(r_max=0.0), dict(lags=(5, 3)), dict(lags=(0,)), dict(lags=tuple(range(1, 10))),
                dict(lags=(2, 2)), dict(box=(0, 1, 2)), dict(box=(1, 1, 0, 1)), dict(frames=(5, 5)), dict(frames=(0, 11), T=10),
                dict(half=True)):
        with pytest.raises(ValueError):
            check_options(**bad)


def test_json_pooled_select_merge(tmp_path):
    from piml_amd.viewstats import ARRAYS, JSON_VERSION, ViewStats, merge
    rng = np.random.default_rng(0)
    m0 = rng.integers(0, 500, (4, G, G))
    st = make(m0, rng.integers(0, 500, (4, G, G)), nn=5, gap=np.arange(GB) * 10, speed=np.linspace(0.5, 1.4, GB), members=3)
    st.map[1] *= 2
    st.focal[2] += 7
    assert JSON_VERSION == 1 and st.members == 3 and st.lags == (0, 8, 16) and st.G == G
    path = tmp_path / 'v.json'
    d = st.to_json(str(path))
    assert d['version'] == 1 and d['options']['lags'] == [8, 16] and d['options']['half'] == HALF
    back = ViewStats.from_json(str(path))
    assert back.options == st.options and all(np.array_equal(getattr(back, k), getattr(st, k)) for k in ARRAYS)
    assert all(np.array_equal(getattr(ViewStats.from_json(d), k), getattr(st, k)) for k in ARRAYS)
    with pytest.raises(ValueError):
        ViewStats.from_json({**d, 'version': 2})
    pool = st.pooled()
    assert pool.members == 1 and np.array_equal(pool.map[0], st.map.sum(0)) and pool.focal[0, 0] == st.focal[:, 0].sum()
    assert np.array_equal(st.member(1).map[0], st.map[1]) and st.member(1).members == 1
    sel = st.select([2, 0, 2])
    assert sel.members == 3 and np.array_equal(sel.focal, st.focal[[2, 0, 2]])
    assert np.array_equal(st.select([0, 1]).pooled().map[0], st.map[:2].sum(0))
    with pytest.raises(IndexError):
        st.select([3])
    mg = merge([st, st.member(0)])
    assert mg.members == 1 and np.array_equal(mg.map[0], st.map.sum(0) + st.map[0]) and mg.options['frames'] == (0, 100)
    assert ViewStats.merge([st, make(m0, opts={**OPTS, 'frames': (0, 50)})]).options['frames'] is None
    with pytest.raises(ValueError):
        merge([st, make(m0, opts={**OPTS, 'cell': 0.25})])
    with pytest.raises(ValueError):
        merge([])
    # the derived quantities are those of the pool
    assert st.front_back_ratio() == pool.front_back_ratio() and np.array_equal(st.g_map(), pool.g_map(), equal_nan=True)


def test_map_density_and_g_map():
    base = np.full((4, G, G), 100, np.int64)
    st = make(base, base * 3)                         # the same share of the pairs in every cell at lag 0 and scrambled
    assert np.allclose(st.map_density(0), 4 * 100 / (4 * G * G * 100 * 0.25)) and st.map_density(0).shape == (G, G)
    assert np.allclose(st.map_density(1, cls='against'), 300 / (4 * G * G * 300 * 0.25))
    assert np.allclose(st.scrambled_map_density(2), st.map_density(1, 2))
    assert np.allclose(st.g_map(), 1.0) and np.allclose(st.g_map(cls=3), 1.0)
    few = base.copy()
    few[:, 0, 0] = 5                                  # 20 pairs in the cell over all classes: below min_count 50
    g = make(few, base * 3).g_map()
    assert math.isnan(g[0, 0]) and np.isfinite(g[1:, 1:]).all()
    assert np.isfinite(make(few, base * 3).g_map(min_count=20)[0, 0])
    assert np.isnan(make(base, opts={**OPTS, 'lags': ()}).pooled().map_density(0)).sum() == 0
    assert np.allclose(st.centres, (np.arange(G) + 0.5 - HALF) * 0.5)


def test_front_back_ratio_of_a_doubled_front():
    """a map with twice the scrambled density ahead and the scrambled density behind: ratio 2"""
    scr = np.full((4, G, G), 60, np.int64)
    m0 = scr.copy()
    m0[:, :, HALF:] *= 2                              # columns: distance ahead; cells ahead of the agent doubled
    total = int(scr.sum())
    st = make(m0, scr, pairs0=total, pairs_s=total)
    assert st.front_back_ratio(r=2.0) == pytest.approx(2.0, abs=1e-12)
    assert st.front_back_ratio(r=1.0) == pytest.approx(2.0, abs=1e-12)
    assert make(scr, scr).front_back_ratio() == pytest.approx(1.0, abs=1e-12)
    assert math.isnan(make(scr, np.zeros_like(scr), pairs_s=0).front_back_ratio())


def test_passing_side_all_left():
    scr = np.zeros((4, G, G), np.int64)
    scr[2] = 50                                       # oncoming scrambled pairs everywhere: chance level 0
    m0 = np.zeros((4, G, G), np.int64)
    m0[2, HALF:HALF + 2, HALF:] = 40                  # class 2, ahead, to the left by less than 1 m
    m0[1, :HALF, HALF:] = 99                          # another class on the right does not count
    side, chance = make(m0, scr).passing_side(width=1.0)
    assert side == 1.0 and chance == 0.0
    m0[2, HALF - 2:HALF, HALF:] = 40                  # as many on the right: 0
    assert make(m0, scr).passing_side()[0] == 0.0
    m0[2, HALF - 2:HALF, HALF:] = 120
    assert make(m0, scr).passing_side()[0] == pytest.approx(-0.5)
    m0[2, :HALF - 2, HALF:] = 1000                    # beyond the width: not counted
    m0[2, :, :HALF] = 1000                            # behind: not counted
    assert make(m0, scr).passing_side()[0] == pytest.approx(-0.5)
    assert math.isnan(make(np.zeros_like(m0), scr).passing_side()[0])


def test_headway_fit_recovers_a_line():
    """Seyfried et al.: gap = 0.36 m + 1.06 s x speed; the table is made from the gap centres"""
    centres = (np.arange(GB) + 0.5) * 0.2
    speed = (centres - 0.36) / 1.06
    gap = np.where(speed > 0, 100 + 10 * np.arange(GB), 0)
    st = make(gap=gap, speed=np.where(speed > 0, speed, 0.0), focal=5000)
    v = st.headway_speed()
    assert np.isnan(v[gap == 0]).all() and np.allclose(v[gap > 0], speed[gap > 0], atol=1e-6)
    m, s = st.headway_fit()
    assert m == pytest.approx(0.36, abs=1e-5) and s == pytest.approx(1.06, abs=1e-5)
    assert st.mean_front_gap() == pytest.approx((gap * centres).sum() / gap.sum())
    assert np.allclose(st.gap_density(), gap / (5000 * 0.2)) and np.allclose(st.gap_centres, centres)
    assert all(math.isnan(x) for x in st.headway_fit(min_count=10 ** 6))
    assert all(math.isnan(x) for x in make().headway_fit())
    nn = make(nn=3, focal=400)
    assert nn.nn_density().shape == (G, G) and nn.nn_density()[0, 3] == pytest.approx(400 / (400 * 0.25)) \
        and nn.nn_density().sum() == pytest.approx(4.0)


def test_compare_view_stats():
    from piml_amd.viewstats import compare_view_stats
    rng = np.random.default_rng(3)
    a = make(rng.integers(60, 500, (4, G, G)), rng.integers(60, 500, (4, G, G)), nn=7,
             gap=np.full(GB, 50), speed=np.linspace(0.4, 1.3, GB))
    c = compare_view_stats(a, a)
    assert set(c) >= {'map_l1', 'g_map_max_diff', 'front_back_diff', 'passing_side_diff', 'nn_map_l1', 'gap_l1',
                      'headway_slope_diff', 'headway_intercept_diff'}
    assert all(c[k] == 0 for k in c if k != 'g_map_cells') and c['g_map_cells'] == G * G
    m0 = np.zeros((4, G, G), np.int64)
    m0[1, 0, 0] = 100
    m1 = np.zeros((4, G, G), np.int64)
    m1[2, 0, 0] = 50                                  # the same cell, another class: disjoint
    d = compare_view_stats(make(m0, nn=1), make(m1, nn=2, gap=np.full(GB, 100), speed=np.ones(GB)))
    assert d['map_l1'] == 1.0 and d['nn_map_l1'] == 1.0 and d['gap_l1'] == 1.0
    assert math.isnan(d['headway_slope_diff']) and d['g_map_max_diff'] == 0.0 and d['g_map_cells'] == 1   # g is over classes
    m1[2, 0, 0] = 40                                  # below min_count: no cell valid in both
    d = compare_view_stats(make(m0), make(m1))
    assert math.isnan(d['g_map_max_diff']) and d['g_map_cells'] == 0
    for key, val in (('cell', 0.25), ('half', 3), ('gap_bins', 5), ('corridor', 0.5), ('cos_same', 0.9), ('v_min', 0.2)):
        with pytest.raises(ValueError):
            compare_view_stats(a, make(opts={**OPTS, key: val}))
    compare_view_stats(a, make(opts={**OPTS, 'lags': (4,), 'frames': None}))          # lags and frames may differ


VIEW_KEYS = ('map_l1', 'nn_map_l1', 'gap_l1', 'front_back_diff', 'passing_side_diff', 'g_map_max_diff', 'headway_slope_diff',
             'headway_intercept_diff')


def _views_pair():
    scr = np.zeros((4, G, G), np.int64)
    scr[:] = 60
    m0 = scr.copy()
    m0[:, :, HALF:] *= 2
    m0[2, HALF:, HALF:] += 30
    ref = make(scr, scr, nn=3)
    sim = make(m0, scr, pairs0=int(scr.sum()), nn=4)
    return sim, ref


def test_stats_objective_view_side():
    from piml_amd import calibrate as C
    from piml_amd.viewstats import compare_view_stats
    assert C.OBJECTIVE_KEYS['views'] == VIEW_KEYS
    assert C.VIEW_DEFAULT_WEIGHTS == {'g_map_max_diff': 0.0, 'headway_slope_diff': 0.0, 'headway_intercept_diff': 0.0}
    sim, ref = _views_pair()
    J, terms = C.stats_objective(views=ref, ref_views=ref)
    assert J == 0.0 and set(VIEW_KEYS) <= set(terms)
    J, terms = C.stats_objective(views=sim, ref_views=ref)                # a views side alone
    want = compare_view_stats(sim, ref, 50)
    assert all(terms[k] == want[k] or (math.isnan(terms[k]) and math.isnan(want[k])) for k in want)
    assert math.isnan(terms['headway_slope_diff']) and math.isfinite(J) and J > 0       # NaN at weight 0 does not count
    assert J == pytest.approx(sum(abs(terms[k]) for k in VIEW_KEYS[:5]), abs=1e-12)
    assert terms['front_back_diff'] > 0.9 and terms['passing_side_diff'] > 0 and terms['nn_map_l1'] == 1.0
    Jw, _ = C.stats_objective(views=sim, ref_views=ref, weights={'g_map_max_diff': 2.0, 'map_l1': 0.0})
    assert Jw == pytest.approx(J - abs(terms['map_l1']) + 2.0 * abs(terms['g_map_max_diff']), abs=1e-12)
    assert C.stats_objective(views=sim, ref_views=ref, weights={'headway_slope_diff': 1.0})[0] == float('inf')
    with pytest.raises(ValueError, match='unknown'):
        C.stats_objective(views=sim, ref_views=ref, weights={'view_l1': 1.0})
    with pytest.raises(ValueError, match='view'):                         # one half of a side is no side
        C.stats_objective(views=sim)


def test_stats_objective_other_sides_unchanged():
    """without a view side the function returns what the other families' comparisons give, as before this family"""
    from test_calibrate_groups import groups
    from test_calibrate_noise import tracks
    from test_calibrate_stats import crowd, pairs
    from piml_amd import calibrate as C
    from piml_amd.crowdstats import compare_crowd_stats
    from piml_amd.groupstats import compare_group_stats
    from piml_amd.pairstats import compare_pair_stats
    from piml_amd.trackstats import compare_track_stats
    sides = dict(crowd=(crowd(1.25), crowd(1.0)), pairs=(pairs(overlap=10), pairs()),
                 groups=(groups(singles=60, pairs_tracks=40), groups()),
                 tracks=(tracks(ac=0.98, acc_bin=0, mean_acc=0.1), tracks(exponent=1.6, straight_bin=18)))
    compare = dict(crowd=compare_crowd_stats, pairs=compare_pair_stats, groups=compare_group_stats,
                   tracks=compare_track_stats)
    weight = lambda k: C.DEFAULT_WEIGHTS.get(k, C.TRACK_DEFAULT_WEIGHTS.get(k, 1.0))       # noqa: E731
    want_J, want_terms = 0.0, {}
    for name, (a, b) in sides.items():
        t = compare[name](a, b, 50)
        want_terms.update(t)
        want_J += sum(weight(k) * abs(t[k]) for k in C.OBJECTIVE_KEYS[name] if t[k] is not None and weight(k) != 0.0)
    kw = {}
    for name, (a, b) in sides.items():
        kw[name], kw['ref_' + name] = a, b
    J, terms = C.stats_objective(**kw)
    assert J == pytest.approx(want_J, abs=1e-12) and math.isfinite(J) and J > 0 and set(terms) == set(want_terms)
    assert not set(terms) & set(VIEW_KEYS)
    assert all(terms[k] == want_terms[k] or (terms[k] != terms[k] and want_terms[k] != want_terms[k]) for k in terms)
    sim, ref = _views_pair()
    Jv, tv = C.stats_objective(views=sim, ref_views=ref)
    Jb, tb = C.stats_objective(**kw, views=sim, ref_views=ref)
    assert Jb == pytest.approx(J + Jv, abs=1e-12) and set(tb) == set(terms) | set(tv)
    assert C.stats_objective(**kw, views=sim)[0] == J                     # one half of the view side: no view side
    Jp, _ = C.stats_objective(kw['crowd'], kw['pairs'], kw['ref_crowd'], kw['ref_pairs'], None, 50, None, None,
                              kw['groups'], kw['ref_groups'], kw['tracks'], kw['ref_tracks'], sim, ref)   # positionally
    assert Jp == Jb


def test_calibrate_accepts_a_six_entry_reference_through_evaluate():
    """the search itself is untouched: with `evaluate` no reference is read, and the CLI knows the views side"""
    from piml_amd import calibrate as C
    a = C.get_args(['--data', 'a.npy', '--match-stats', '--match', 'crowd,pairs,views'])
    assert a.match == ('crowd', 'pairs', 'views')
    with pytest.raises(SystemExit):
        C.get_args(['--data', 'a.npy', '--match-stats', '--match', 'crowd,view'])
    assert C.get_args(['--data', 'a.npy', '--match-stats']).match == ('crowd', 'pairs')


def test_cli_parsing():
    from piml_amd import simulate, viewstats
    a = viewstats.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'r.npy', '--box', 'auto', '--frames', '3:400',
                            '--lags', '8,16', '--cell', '0.5', '--half', '8', '--out', 'o.json'])
    assert a.data == ['a.npy', 'b.npy'] and a.ref == 'r.npy' and a.box == 'auto' and a.frames == (3, 400)
    assert a.lags == (8, 16) and a.cell == 0.5 and a.half == 8 and a.gap_bins == 60 and a.out == 'o.json'
    d = viewstats.get_args(['--data', 'a.npy', '--box', '5,25,15,35'])
    assert d.box == (5.0, 25.0, 15.0, 35.0) and d.lags == (64, 128, 192) and d.frames is None and d.half == 12
    for bad in (['--data', 'a.npy', '--lags', '5,3'], ['--data', 'a.npy', '--half', '17'], ['--data', 'a.npy', '--box', '1,2'],
                ['--data', 'a.npy', '--frames', '5:5'], ['--data', 'a.npy', '--gap_bins', '300'], ['--lags', '1']):
        with pytest.raises(SystemExit):
            viewstats.get_args(bad)
    own, _ = simulate.get_args(['--seeds', '0:2', '--view-stats', 'v.json', '--view-lags', '4,8', '--frames', '40'])
    assert own.view_stats == 'v.json' and own.view_lags == (4, 8) and own.pair_stats is None and own.seeds == [0, 1]
    own, _ = simulate.get_args(['--frames', '40'])
    assert own.view_stats is None and own.view_lags == (64, 128, 192)
    with pytest.raises(SystemExit):
        simulate.get_args(['--view-stats', 'v.json', '--view-lags', '8,4'])


def test_library_exports_and_rejects_bad_arguments():
    from test_abi import declared_symbols
    from piml_amd import _lib, ops_metrics
    assert {'piml_view_stats', 'piml_view_stats_workspace_bytes'} <= set(declared_symbols())
    assert {'piml_view_stats', 'piml_view_stats_workspace_bytes'} <= set(_lib.SIGNATURES)
    assert (ops_metrics.VIEW_MAX_HALF, ops_metrics.VIEW_MAX_BINS, ops_metrics.VIEW_MAX_LAGS) == (16, 256, 8)
    L = _lib.lib()
    fake = 1 << 20          # never dereferenced: every call below is refused before any HIP call
    good = (ctypes.c_int * 3)(4, 8, 12)
    nine = (ctypes.c_int * 9)(*range(1, 10))

    def call(S=1, T=20, N=3, t0=0, t1=20, lags=good, K=3, v_min=0.1, cell=0.25, half=12, cs=0.7, rmax=0.0, corridor=0.4,
             gb=0.1, GB_=60, box=0, x1=1., y0=0., nul=fake, wsb=1 << 24):
        lp = None if lags is None else ctypes.addressof(lags)
        return L.piml_view_stats(nul, fake, fake, None, S, T, N, t0, t1, lp, K, v_min, cell, half, cs, rmax, corridor, gb,
                                 GB_, box, 0., x1, y0, 1., fake, fake, fake, fake, fake, fake, fake, wsb, None)
    for bad in (dict(half=0), dict(half=17), dict(GB_=257), dict(GB_=0), dict(lags=nine, K=9), dict(K=-1),
                dict(lags=(ctypes.c_int * 3)(12, 8, 4)), dict(lags=(ctypes.c_int * 3)(4, 4, 12)),
                dict(lags=(ctypes.c_int * 3)(0, 4, 8)), dict(lags=None), dict(wsb=8),
                dict(wsb=L.piml_view_stats_workspace_bytes(1, 3, 12, 60) - 1), dict(S=0), dict(T=0), dict(N=0), dict(N=65537),
                dict(t0=20), dict(t1=21), dict(t0=-1), dict(t0=5, t1=5), dict(v_min=0.0), dict(cell=float('inf')),
                dict(cs=1.5), dict(cs=float('nan')), dict(rmax=float('nan')), dict(corridor=0.0), dict(gb=-0.1),
                dict(box=1, x1=0.), dict(box=1, y0=2.), dict(nul=None)):
        assert call(**bad) == 1, bad
    assert L.piml_view_stats_workspace_bytes(2, 3, 5, 7) == 2 * (2 * 4 + 4 * 4 * 100 + 101 + 8 + 7) * 8
    assert L.piml_view_stats_workspace_bytes(2, -1, 5, 7) == -1


def test_operator_refuses_cpu_tensors():
    import torch
    from piml_amd import _lib, ops_metrics
    P = torch.zeros(1, 4, 3, 2)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.view_stats_frames(P, P, torch.ones(1, 4, 3))


def test_run_shapes_hold():
    """the run = 3 and run = VS_MAX_RUN shapes of test_viewstats_gpu.py, derived from the constants of viewstats.hip"""
    SH.check_run_shapes()
    assert SH.constant('VS_TILE') == 1024 and SH.constant('VS_MAX_GRID') == 1 << 20
    c = SH.MID['base']
    assert (c['S'], c['T'], c['N'], c['lags']) == (7, 331, 24, (1, 7))
    assert SH.offsets(331, (1, 7, 400)) == [0, 331, 661, 985, 985]


def test_restatement_on_the_analytic_scene():
    """the restatement's float64 and float32 runs agree on the scene of the GPU test, without an ambiguous pair"""
    P, V = np.array(SH.SCENE_P, np.float32)[None], np.array(SH.SCENE_V, np.float32)[None]
    M = np.ones((1, len(SH.SCENE_P)), np.float32)
    w = REF.view_stats(P, V, M, lags=())
    assert w['n_ambiguous'] == 0 and w['focal'].tolist() == [[5]] and w['pairs'].tolist() == [[25]]
    assert all(np.array_equal(w[k], w['f32'][k]) for k in REF.OUTPUTS)
    r = REF.view_stats(SH.rotate(P), SH.rotate(V), M, lags=())
    assert all(np.array_equal(w[k], r[k]) for k in REF.OUTPUTS)
    only0 = REF.view_stats(P, V, M, lags=(), box=(-0.5, 0.5, -0.5, 0.5))
    assert only0['map'][0, 0, 2, 13, 20] == 1 and only0['nn_map'][0, 12 * 24 + 15] == 1 and only0['front_gap'][0, 9] == 1


@pytest.mark.parametrize('N,S,T', SH.CASES)
def test_ambiguous_share_of_the_random_cases(N, S, T):
    """the cap is a condition of the GPU tests' inputs, checked here: at most CAP of the pairs are ambiguous"""
    for which in range(3):
        want = SH.case_reference(N, S, T, which)
        share = SH.ambiguous_share(want)
        print(f'[viewstats] N={N} S={S} T={T} set {which}: {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous '
              f'({share:.2e})')
        assert share <= SH.CAP, (which, share)
        if N >= 300:
            assert want['n_pairs'] > 0


def test_ambiguous_share_of_the_run_shapes_and_clips():
    for name, variant in SH.MID_CALLS:
        share = SH.ambiguous_share(SH.mid_reference(name, variant))
        print(f'[viewstats] run = 3, {name} {variant}: ambiguous share {share:.2e}')
        assert share <= SH.CAP, (name, variant, share)
    for name, box in SH.CLIPS:
        share = SH.ambiguous_share(SH.clip_reference(name, box))
        print(f'[viewstats] {name}: ambiguous share {share:.2e}')
        assert share <= SH.CAP, (name, share)
