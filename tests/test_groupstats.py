"""CPU: the numpy restatement of the group statistics (groupstats_ref.py) against hand counts on multiples of 1/8 m, its
ambiguity share on every generator case and on the recorded clips, the host half on hand-made integer rows (chains, the
integer share rule at its boundary, an ineligible track, the cap at g_max), the GroupStats container (pooled / select / merge
/ JSON), the comparison and its refusals, the option checks of group_stats and of the command lines, and the C entries'
argument refusals (no compute call without a GPU)."""
import functools
import json
import os

import numpy as np
import pytest

import groupstats_ref as REF
from conftest import GOLDEN, REPO

Q = REF.Q
CAP = 1e-3                                    # the ambiguous share of items, as the siblings'
GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35'
UCY_CLIP = 'UCY_Dataset_time162-216_timeunit0.08'
TILE = 256                                    # PIML_GROUP_TILE, the focal frames staged per LDS tile
CASES = [(1, 1, 1), (2, 1, 2), (65, 3, 40), (300, 2, 12), (3, 1, 2 * TILE + 5)]       # N, S, T


def option_sets(S, T, N):
    """the three option sets of a random case: the defaults with min_time scaled to T (min_frames = max(1, (T - 1) // 3); one
    frame when T = 2: min_time = dt); a window + n_active per member + other radii and bin widths; one bin each"""
    k = max(1, (T - 1) // 3)
    scaled = 0.08 if T == 2 else (k - 0.5) * 0.08
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    window = dict(frames=(1, T)) if T > 2 else {}
    return (dict(min_time=scaled),
            dict(n_active=n_active, dt=0.1, radius=1.2, dv_max=0.8, v_min=0.05, share=0.7, min_time=(k - 0.5) * 0.1, r_bin=0.25,
                 r_bins=7, a_bins=4, **window),
            dict(min_time=scaled, r_bin=0.5, r_bins=1, a_bins=1))


@functools.lru_cache(maxsize=None)
def planted_case(N, S, T):
    """the generator case and its restatement under the three option sets, made once: (P, M, plans, [(kw, want)])"""
    P, M, plans = REF.planted_tracks(S, T, N, seed=N + T)
    return P, M, plans, [(kw, REF.group_stats(P, M, **kw)) for kw in option_sets(S, T, N)]


def assert_cap(want, label):
    frac = want['n_ambiguous'] / max(want['n_items'], 1)
    print(f'\n[groupstats] {label}: {want["n_items"]} items, {want["n_ambiguous"]} ambiguous ({frac:.2e})')
    assert frac <= CAP, (label, frac)


def _load_clip(name):
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return raw


@functools.lru_cache(maxsize=None)
def clip_case(name):
    raw = _load_clip(name)
    P, M = raw.position.numpy(), raw.mask_p.numpy()
    return raw, P, M, REF.group_stats(P, M, dt=float(raw.time_unit))


def stats_of(want, T, S, **kw):
    """a GroupStats from the restatement's float32 run and the package's host half (no device)"""
    from piml_amd import groupstats as GS
    o = dict(GS.DEFAULTS)
    o.update({k: v for k, v in kw.items() if k in o})
    frames = kw.get('frames') or (0, T)
    opts = GS.make_options(frames=frames, **o)
    assert (opts['min_frames'], opts['share_q']) == (want['min_frames'], want['share_q'])
    arrays = {k: want[k] for k in ('edges', 'n_edges') + REF.PAIR_ROWS + REF.MEMBER_ROWS}
    arrays.update(GS.host_rows(arrays, opts['min_frames'], opts['share_q']))
    arrays['slices'] = np.full(S, frames[1] - frames[0], np.int64)
    return GS.GroupStats(arrays, opts)


def test_reference_against_hand_counts():
    P, M, kw, hand = REF.analytic_scene()
    want = REF.group_stats(P, M, **kw)
    assert want['n_items'] == 15 * 39 and want['n_ambiguous'] == 0 and want['min_frames'] == 25 and want['share_q'] == 819
    for k in REF.OUTPUTS:
        assert np.array_equal(want[k], hand[k]), (k, want[k], hand[k])
        assert np.array_equal(want['f64'][k], hand[k]), (k, 'float64 run')
    st = stats_of(want, 40, 1, **kw)
    for k in REF.HOST_ROWS:
        assert np.array_equal(getattr(st, k), hand[k]), k
    assert st.groups(0) == [[0, 1, 2]] and st.eligible_tracks() == 6 and st.group_fraction() == 0.5
    assert st.size_distribution().tolist() == [0, 0.5, 0, 0.5, 0, 0, 0, 0, 0]
    dt = float(np.float32(0.08))
    speed = st.speed_by_size()
    assert speed[3] == (3 * 39 * (Q // 8)) / float(Q) / dt / (3 * 39) and speed[3] == pytest.approx(1.5625)
    assert speed[1] == (2 * 39 * (Q // 8)) / float(Q) / dt / (3 * 39) and np.isnan(speed[2])
    assert st.speed_ratio() == pytest.approx(1.5) and st.abreast_density().tolist() == [10 / 3, 0, 0, 0, 0, 0, 0, 0, 10 / 3, 10 / 3]
    assert st.mean_member_distance() == pytest.approx((2.5 + np.sqrt(3.25)) / 3, abs=1e-6)
    assert st.member_distance_density()[[8, 12, 14]].tolist() == [1 / 3 / 0.125] * 3
    # the members alone, and what breaks a link
    assert REF.group_stats(P[:, :, 3:], M[:, :, 3:], **kw)['together'][0] == 0                 # 3, 4, 5: nobody together
    short = REF.group_stats(P, M, frames=(0, 25), **kw)                                        # 24 steps < min_frames
    assert short['candidates'][0] == 0 and short['together'][0] == 3 * 24 and (short['group_id'] == -1).all()
    M2 = M.copy()
    M2[0, 20, 1] = 0.5                                                                         # agent 1 misses a frame
    gap = REF.group_stats(P, M2, **kw)
    assert gap['edges'].tolist() == [[0, 0, 1, 37, 37], [0, 0, 2, 39, 39], [0, 1, 2, 37, 37]] and gap['trk_steps'][0, 1] == 37
    far = REF.group_stats(P, M, radius=1.25, **kw)                                             # 1.5 m and 1.8 m are apart now
    assert far['edges'].tolist() == [[0, 0, 1, 39, 39]] and far['group_id'][0].tolist() == [0, 0, 2, 3, 4, 5]
    few = REF.group_stats(P, M, n_active=[2], **kw)
    assert few['pairs'][0] == 39 and few['group_id'][0].tolist() == [0, 0, -1, -1, -1, -1]


def test_host_half_on_hand_made_rows():
    from piml_amd.groupstats import host_rows
    q = 819
    steps = np.array([[30, 30, 30, 30, 30, 5, 30, 30], [40] * 8])
    path = np.arange(16).reshape(2, 8) * 1000 + 7
    # member 0: a chain 0-1, 1-2 (0 and 2 never together); 3-4 exactly at the share boundary (near 1024 == 819 co: a link);
    # 6-7 one together frame short of it (a candidate only); track 5 has 5 steps: ineligible
    edges = np.array([[0, 0, 1, 30, 30], [0, 1, 2, 25, 24], [0, 3, 4, 1024, 819], [0, 6, 7, 1024, 818]])
    rows = dict(edges=edges, trk_steps=steps[:1], trk_path=path[:1])
    h = host_rows(rows, 10, q)
    mine = REF.host_rows(edges, steps[:1], path[:1], 10, q)
    for k in REF.HOST_ROWS:
        assert np.array_equal(h[k], mine[k]), k
    assert h['candidates'].tolist() == [4] and h['links'].tolist() == [3]
    assert h['group_id'].tolist() == [[0, 0, 0, 3, 3, -1, 6, 7]] and h['group_id'].dtype == np.int32
    assert h['size_tracks'].tolist() == [[0, 2, 2, 3, 0, 0, 0, 0, 0]]
    assert h['size_path'][0, 3] == path[0, :3].sum() and h['size_path'][0, 1] == path[0, 6:].sum()
    assert h['size_steps'].tolist() == [[0, 60, 60, 90, 0, 0, 0, 0, 0]] and h['size_tracks'][0].sum() == 7
    # share 1: only a pair that is always together; share_q 1 (share ~ 0.001): every candidate
    assert host_rows(rows, 10, 1024)['links'].tolist() == [1] and host_rows(rows, 10, 1)['links'].tolist() == [4]
    # two members; member 1: ten tracks would be capped at g_max = 8 -- here all eight in one chain, given out of order
    chain = np.array([[1, 6, 7, 40, 40], [1, 0, 1, 40, 40], [1, 2, 3, 40, 40], [1, 1, 2, 40, 40], [1, 4, 5, 40, 40], [1, 3, 4, 40, 40],
                      [1, 5, 6, 40, 40]])
    both = dict(edges=np.concatenate([edges, chain]), trk_steps=steps, trk_path=path)
    h = host_rows(both, 10, q)
    mine = REF.host_rows(both['edges'], steps, path, 10, q)
    for k in REF.HOST_ROWS:
        assert np.array_equal(h[k], mine[k]), k
    assert h['size_tracks'][1].tolist() == [0] * 8 + [8] and (h['group_id'][1] == 0).all() and h['links'].tolist() == [3, 7]
    capped = host_rows(both, 10, q, g_max=3)
    assert capped['size_tracks'].tolist() == [[0, 2, 2, 3], [0, 0, 0, 8]] and capped['size_steps'][1, 3] == 320
    assert np.array_equal(REF.host_rows(both['edges'], steps, path, 10, q, 3)['size_tracks'], capped['size_tracks'])
    none = host_rows(dict(edges=np.zeros((0, 5), np.int64), trk_steps=steps, trk_path=path), 10, q)
    assert none['size_tracks'][:, 1].tolist() == [7, 8] and none['links'].tolist() == [0, 0]


@pytest.mark.parametrize('N,S,T', CASES)
def test_generator_cases_stay_within_the_ambiguity_cap(N, S, T):
    P, M, plans, runs = planted_case(N, S, T)
    assert P.shape == (S, T, N, 2) and M.shape == (S, T, N) and P.dtype == M.dtype == np.float32
    for kw, want in runs:
        assert_cap(want, f'N={N} S={S} T={T} {sorted(kw)}')
        assert want['together'].sum() <= want['pairs'].sum() == want['n_items']
    want = runs[0][1]
    if N >= 65:
        kinds = {k for plan in plans for k, _ in plan}
        assert kinds == set(REF.KINDS) and not np.isfinite(P).all() and (M == 0.5).any()
        for s, plan in enumerate(plans):
            links = {(i, j) for m, i, j, co, near in want['edges'].tolist() if m == s and near * 1024 >= want['share_q'] * co}
            cands = {(i, j) for m, i, j, co, near in want['edges'].tolist() if m == s}
            for kind, slots in plan:
                a, b = sorted(slots[:2])
                if kind == 'short':
                    assert (a, b) not in cands, (s, kind, slots)           # together for less than min_time
                if kind == 'lowshare' and (a, b) in cands:
                    assert (a, b) not in links, (s, kind, slots)           # together for less than `share` of the common frames
                if kind == 'chain' and {tuple(sorted((slots[0], x))) for x in slots[1:]} <= links:
                    assert tuple(sorted(slots[1:])) not in cands           # i-j and j-k linked, i-k apart
        assert any(kind == 'chain' and {tuple(sorted((slots[0], x))) for x in slots[1:]}
                   <= {(i, j) for m, i, j, *_ in want['edges'].tolist() if m == s}
                   for s, plan in enumerate(plans) for kind, slots in plan)
        assert any(kind == 'lowshare' and tuple(sorted(slots)) in {(i, j) for m, i, j, *_ in want['edges'].tolist() if m == s}
                   for s, plan in enumerate(plans) for kind, slots in plan)


def test_recorded_clips_through_the_restatement():
    for name in (GC_CLIP, UCY_CLIP):
        raw, P, M, want = clip_case(name)
        assert_cap(want, name[:3])
        assert want['links'][0] >= 1 and want['size_tracks'][0, 2:].sum() >= 2 and want['link_frames'][0] > 0
        assert want['dist'].sum() == want['link_frames'].sum() == want['abreast'].sum() + want['abreast_skipped'].sum()
        print(f'[groupstats] {name[:3]}: {int(want["size_tracks"].sum())} eligible tracks, {int(want["links"][0])} links, tracks by '
              f'group size {want["size_tracks"][0, 1:].tolist()}')


def test_container_pooled_select_merge_json(tmp_path):
    from piml_amd import groupstats as GS
    P, M, plans, runs = planted_case(65, 3, 40)
    kw, want = runs[0]
    st = stats_of(want, 40, 3, **kw)
    for k in REF.HOST_ROWS:
        assert np.array_equal(getattr(st, k), want[k]), k
    assert st.members == 3 and st.links.sum() > 0 and st.trk_steps.shape == (3, 65) and (st.slices == 40).all()
    pool = st.pooled()
    assert pool.members == 1 and pool.edges is None and pool.group_id is None and pool.slices[0] == 120
    for k in GS.ADDITIVE:
        assert np.array_equal(getattr(pool, k)[0], getattr(st, k).sum(0)), k
    with pytest.raises(ValueError):
        pool.groups(0)
    sel = st.select([2, 0, 0])
    assert sel.members == 3 and np.array_equal(sel.dist[1], st.dist[0]) and np.array_equal(sel.group_id[0], st.group_id[2])
    assert np.array_equal(sel.edges[sel.edges[:, 0] == 0][:, 1:], st.edges[st.edges[:, 0] == 2][:, 1:])
    assert np.array_equal(sel.edges[sel.edges[:, 0] == 2][:, 1:], st.edges[st.edges[:, 0] == 0][:, 1:])
    assert st.member(1).edges[:, 0].max() == 0 and np.array_equal(st.member(1).abreast, st.abreast[1:2])
    with pytest.raises(IndexError):
        st.select([3])
    for m in range(3):
        groups = st.groups(m)
        assert groups and all(len(g) >= 2 and g == sorted(g) for g in groups)
        assert sum(len(g) for g in groups) == st.size_tracks[m, 2:].sum()
        assert all((st.group_id[m, g] == g[0]).all() for g in groups)
    assert any(len(g) == 3 for m in range(3) for g in st.groups(m))
    merged = GS.merge([st.member(0), st.member(1), st.member(2)])
    for k in GS.ADDITIVE:
        assert np.array_equal(getattr(merged, k), getattr(pool, k)), k
    assert GS.GroupStats.merge([st, st]).links[0] == 2 * pool.links[0]
    short = stats_of(REF.group_stats(P[:1, :20], M[:1, :20], **kw), 20, 1, **kw)
    mixed = GS.merge([st, short])
    assert mixed.options['frames'] is None and mixed.slices[0] == 140 and 0 < mixed.group_fraction() < 1
    assert st.group_fraction() == pool.size_tracks[0, 2:].sum() / pool.size_tracks[0].sum()
    assert st.size_distribution().sum() == pytest.approx(1.0) and np.isfinite(st.speed_ratio())
    assert st.member_distance_density().sum() * 0.1 == pytest.approx(pool.dist[0, :-1].sum() / pool.dist[0].sum())
    assert st.abreast_density().mean() == pytest.approx(1.0) and 0.4 < st.mean_member_distance() < 2.0
    path = str(tmp_path / 'groups.json')
    d = st.to_json(path)
    back = GS.GroupStats.from_json(path)
    assert back.options == st.options
    for k in GS.ARRAYS:
        assert np.array_equal(getattr(back, k), getattr(st, k)), k
    assert json.dumps(back.to_json()) == json.dumps(d)
    assert GS.GroupStats.from_json(pool.to_json()).edges is None
    assert d['pooled']['links'] == int(st.links.sum()) and d['pooled']['eligible_tracks'] == st.eligible_tracks()
    with pytest.raises(ValueError):
        GS.GroupStats.from_json({**d, 'version': 99})
    with pytest.raises(ValueError):
        GS.merge([])


def test_compare_group_stats_and_its_refusals():
    from piml_amd import groupstats as GS
    P, M, kw, hand = REF.analytic_scene()
    a = stats_of(REF.group_stats(P, M, **kw), 40, 1, **kw)
    # b: agent 2 walks 1 m behind agent 0 instead of 1.5 m, and agent 5 walks along with agent 4
    P2 = P.copy()
    P2[0, :, 2, 0] += 0.5
    P2[0, :, 5, 0] = P[0, :, 4, 0] + 0.5
    b = stats_of(REF.group_stats(P2, M, **kw), 40, 1, **kw)
    assert b.groups(0) == [[0, 1, 2], [4, 5]] and b.size_tracks[0].tolist() == [0, 1, 2, 3, 0, 0, 0, 0, 0]
    c = GS.compare_group_stats(a, b, min_count=1)
    assert set(c) == {'group_fraction_diff', 'size_l1', 'member_distance_l1', 'abreast_l1', 'speed_ratio_diff'}
    assert c['group_fraction_diff'] == pytest.approx(5 / 6 - 1 / 2) and c['size_l1'] == pytest.approx(1 / 3 + 1 / 3)
    # distance shares: a 1/3 each in bins 8, 12, 14; b 1/4 in bins 5 (4-5, sqrt 0.5 m) and 11 (1-2, sqrt 2 m), 1/2 in bin 8 (0-1 and 0-2, 1 m)
    assert c['member_distance_l1'] == pytest.approx(1 / 4 + (1 / 2 - 1 / 3) + 1 / 4 + 1 / 3 + 1 / 3)
    assert 0 < c['abreast_l1'] <= 2 and c['speed_ratio_diff'] == pytest.approx(1.5 - 1.0)
    same = GS.compare_group_stats(a, a, min_count=1)
    assert all(v == 0 for v in same.values())
    high = GS.compare_group_stats(a, b, min_count=7)
    assert np.isnan(high['group_fraction_diff']) and np.isnan(high['size_l1']) and np.isnan(high['speed_ratio_diff'])
    assert np.isfinite(high['member_distance_l1']) and np.isfinite(high['abreast_l1'])
    assert all(np.isnan(v) for v in GS.compare_group_stats(a, b, min_count=1000).values())
    for key, val in (('radius', 1.5), ('dt', 0.1), ('share', 0.7), ('min_time', 1.0), ('r_bin', 0.25), ('a_bins', 5)):
        other = stats_of(REF.group_stats(P, M, **{**kw, key: val}), 40, 1, **{**kw, key: val})
        with pytest.raises(ValueError, match='options'):
            GS.compare_group_stats(a, other)
        with pytest.raises(ValueError):
            GS.merge([a, other])


def test_option_validation_of_group_stats_and_the_command_lines(capsys):
    from piml_amd import groupstats as GS
    from piml_amd import ops_metrics, simulate
    assert GS.check_options() is None and GS.check_options(frames=(2, 5), T=5) == (2, 5)
    inf, nan = float('inf'), float('nan')
    for kw in (dict(dt=0), dict(dt=nan), dict(radius=0), dict(radius=-1), dict(radius=inf), dict(radius=2000), dict(radius=True),
               dict(dv_max=0), dict(dv_max=1e-30), dict(v_min=-0.1), dict(v_min=nan), dict(min_time=0), dict(min_time=inf),
               dict(share=0), dict(share=1.5), dict(share=nan), dict(r_bin=0), dict(r_bins=0), dict(r_bins=257), dict(a_bins=0),
               dict(a_bins=257), dict(a_bins=2.5), dict(frames=(3, 3)), dict(frames=(-1, 2)), dict(frames=(0, 9), T=8),
               dict(N=65537, T=4), dict(T=(1 << 25) + 1), dict(max_edges=0), dict(max_edges=1.5), dict(radius=1000, N=65536, T=1 << 25)):
        with pytest.raises(ValueError):
            GS.check_options(**kw)
    assert GS.check_options(v_min=0, share=1, max_edges=7) is None
    r2, dv2, vm2, min_frames, share_q = ops_metrics.group_thresholds(0.08, 2.0, 0.5, 0.1, 2.0, 0.8)
    assert (r2, min_frames, share_q) == (4.0, 25, 819) and dv2 == float(np.float32(0.04 ** 2)) and vm2 == float(np.float32(0.008 ** 2))
    assert tuple(float(x) for x in REF.thresholds()[:3]) == (r2, dv2, vm2) and REF.thresholds()[3:] == (25, 819)
    assert ops_metrics.group_thresholds(0.08, 2.0, 0.5, 0.1, 0.08, 0.8)[3] == 1
    assert ops_metrics.group_thresholds(0.08, 2.0, 0.5, 0.1, 0.001, 0.8)[3] == 1
    # refused on the host before anything touches a device
    P, M = np.zeros((2, 3, 2), np.float32), np.ones((2, 3), np.float32)
    for kw in (dict(radius=0), dict(frames=(0, 3)), dict(share=2), dict(max_edges=-1)):
        with pytest.raises(ValueError):
            GS.group_stats(P, M, **kw)
    args = GS.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'c.npy', '--frames', '2:9', '--radius', '1.5', '--dv-max', '0.4',
                        '--min-time', '1.0', '--share', '0.75', '--out', 'g.json'])
    assert (args.frames, args.radius, args.dv_max, args.min_time, args.share, args.v_min) == ((2, 9), 1.5, 0.4, 1.0, 0.75, 0.1)
    for argv in (['--data', 'a.npy', '--radius', '0'], ['--data', 'a.npy', '--share', '1.1'], ['--data', 'a.npy', '--frames', '5:5'],
                 ['--radius', '1']):
        with pytest.raises(SystemExit) as ex:
            GS.get_args(argv)
        assert ex.value.code == 2, argv
    capsys.readouterr()
    own, _ = simulate.get_args(['--group-stats', 'groups.json'])
    assert own.group_stats == 'groups.json' and simulate._stats_path(own) == 'groups.json'


def _pairs(L, S=1, T=4, N=8, t0=0, t1=4, r2=4.0, dv2=0.0016, vm2=6.4e-5, min_frames=2, max_edges=4):
    return L.piml_group_pairs(None, None, None, S, T, N, t0, t1, r2, dv2, vm2, min_frames, max_edges, *([None] * 6), None)


def _members(L, S=1, T=4, N=8, t0=0, t1=4, n_links=1, r2=4.0, dv2=0.0016, vm2=6.4e-5, r_bin=0.1, r_bins=20, a_bins=10):
    return L.piml_group_members(None, None, S, T, N, t0, t1, None, n_links, r2, dv2, vm2, r_bin, r_bins, a_bins, *([None] * 5), None)


def test_entries_refuse_bad_arguments_without_gpu():
    from piml_amd import _lib, ops_metrics
    from test_abi import declared_symbols
    assert _lib.ABI_VERSION == 35
    assert {'piml_group_pairs', 'piml_group_members'} <= set(declared_symbols(('piml_hip.h',))) & set(_lib.SIGNATURES)
    header = open(os.path.join(REPO, 'include', 'piml_hip.h')).read()
    assert f'#define PIML_GROUP_TILE {TILE}\n' in header
    L = _lib.lib()
    assert (ops_metrics.GROUP_MAX_N, ops_metrics.GROUP_MAX_FRAMES, ops_metrics.GROUP_MAX_BINS, ops_metrics.GROUP_Q,
            ops_metrics.GROUP_TILE, ops_metrics.GROUP_MAX_EDGES) == (65536, 1 << 25, 256, Q, TILE, 1 << 20)
    inf, nan = float('inf'), float('nan')
    common = (dict(S=-1), dict(T=-1, t1=0), dict(N=-1), dict(N=65537), dict(t0=-1), dict(t1=5), dict(t0=3, t1=2), dict(r2=0.0),
              dict(r2=nan), dict(r2=inf), dict(dv2=0.0), dict(dv2=-1.0), dict(dv2=nan), dict(vm2=-1.0), dict(vm2=nan), dict(vm2=inf),
              dict(T=(1 << 25) + 1, t1=(1 << 25) + 1),                                 # the window's length
              dict(r2=1e6, N=65536, T=1 << 25, t1=1 << 25))                            # sqrt(r2) Q N^2 / 2 T' >= 2^63
    for call, extra in ((_pairs, (dict(min_frames=0), dict(max_edges=-1))),
                        (_members, (dict(n_links=-1), dict(r_bin=0.0), dict(r_bin=nan), dict(r_bin=inf), dict(r_bins=0),
                                    dict(r_bins=257), dict(a_bins=0), dict(a_bins=257)))):
        for kw in common + extra:
            assert call(L, **kw) == 1, (call.__name__, kw)
        assert call(L) == 1                                                            # a NULL pointer where there is work
        for kw in (dict(S=0), dict(t0=2, t1=2), dict(N=0), dict(T=0, t1=0)):           # empty problems
            assert call(L, **kw) == 0, (call.__name__, kw)
    assert _members(L, n_links=0) == 1 and _pairs(L, max_edges=0) == 1                 # the outputs are still needed


def test_operators_refuse_cpu_tensors():
    import torch
    from piml_amd import _lib, ops_metrics
    P, M = torch.zeros(1, 3, 4, 2), torch.ones(1, 3, 4)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.group_stats_frames(P, M, 0.08)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.group_pairs_frames(P, M, 4.0, 0.0016, 6.4e-5, 2)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.group_members_frames(P, M, torch.zeros(1, 3, dtype=torch.int32), 4.0, 0.0016, 6.4e-5)
