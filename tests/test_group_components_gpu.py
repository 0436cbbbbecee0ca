"""GPU: the host half of the group statistics on the device (piml_group_components) against the numpy
restatement groupstats_ref.host_rows on hand-made integer rows -- the smallest shapes, chains in the worst row orders, a
star, the share rule at its boundary, saturated sizes, an ineligible track, rows past the count and past the capacity, one
large case --, the whole statistics with components='device' against components='host' on the generator cases and the
recorded clips, determinism and graph replay, and the group side of the statistics fit: the evaluator's terms against
stats_objective by hand, and a tiny fit of Ag.  Every comparison of the kernel is integer equality."""
import functools

import numpy as np
import pytest
import torch

import groupstats_ref as REF
from test_groupstats import CASES, GC_CLIP, UCY_CLIP, clip_case, planted_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROWS = REF.HOST_ROWS                          # candidates, links, group_id, size_tracks, size_path, size_steps
Q819 = 819                                    # round(0.8 * 1024)
SENTINEL = -7


def run(edges, n_edges, steps, path, min_frames=10, share_q=Q819, g_max=8):
    """the operator on numpy rows: edges (S, cap, 4), n_edges (S), steps / path (S, N) -> dict of numpy arrays"""
    from piml_amd import ops_metrics
    out = ops_metrics.group_components_frames(torch.tensor(np.asarray(edges, np.int32).reshape(len(n_edges), -1, 4), device=DEV),
                                              torch.tensor(np.asarray(n_edges, np.int32), device=DEV),
                                              torch.tensor(np.asarray(steps, np.int64), device=DEV),
                                              torch.tensor(np.asarray(path, np.int64), device=DEV), min_frames, share_q, g_max)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def want_of(edges, n_edges, steps, path, min_frames=10, share_q=Q819, g_max=8):
    """the restatement on the rows the kernel may read: the first min(n_edges, cap) of each member"""
    edges = np.asarray(edges, np.int64).reshape(len(n_edges), -1, 4)
    rows = [[s, *r] for s in range(len(n_edges)) for r in edges[s, :min(int(n_edges[s]), edges.shape[1])].tolist()]
    want = REF.host_rows(np.array(rows, np.int64).reshape(-1, 5), np.asarray(steps, np.int64), np.asarray(path, np.int64),
                         min_frames, share_q, g_max)
    want['candidates'] = np.asarray(n_edges, np.int64)             # the true count, also past the capacity
    return want


def check(edges, n_edges, steps, path, label, **kw):
    from piml_amd.groupstats import host_rows
    got, want = run(edges, n_edges, steps, path, **kw), want_of(edges, n_edges, steps, path, **kw)
    assert not got['status'].any(), label
    for k in ROWS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (label, k, got[k], want[k])
    e3 = np.asarray(edges, np.int64).reshape(len(n_edges), -1, 4)
    if all(int(n) <= e3.shape[1] for n in n_edges):                # and the package's own host half, where it can be asked
        flat = np.array([[s, *r] for s in range(len(n_edges)) for r in e3[s, :int(n_edges[s])].tolist()], np.int64).reshape(-1, 5)
        own = host_rows(dict(edges=flat, trk_steps=np.asarray(steps, np.int64), trk_path=np.asarray(path, np.int64)),
                        kw.get('min_frames', 10), kw.get('share_q', Q819), kw.get('g_max', 8))
        for k in ROWS:
            assert np.array_equal(got[k], own[k]), (label, k, 'host_rows')
    return got


def tracks(N, S=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(10, 60, (S, N)), rng.integers(1, 1 << 40, (S, N))


def link(i, j, co=30, near=30):
    return [min(i, j), max(i, j), co, near]


def test_smallest_shapes():
    st, pa = tracks(1)
    got = check(np.zeros((1, 0, 4)), [0], st, pa, 'N = 1, no edge')
    assert got['group_id'].tolist() == [[0]] and got['size_tracks'][0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    st, pa = tracks(2)
    got = check([[link(0, 1)]], [1], st, pa, 'N = 2, one link')
    assert got['group_id'].tolist() == [[0, 0]] and got['links'].tolist() == [1] and got['size_tracks'][0, 2] == 2
    assert got['size_path'][0, 2] == pa.sum() and got['size_steps'][0, 2] == st.sum()
    # N = 257 slots and cap = 257 rows: one past the workgroup's 256 lanes in the loops over the rows and over the slots;
    # the last row and the last slot belong to the lane that wraps
    N = 257
    st, pa = tracks(N, seed=1)
    rows = [link(k, k + 1) for k in range(0, 256, 2)] + [link(2 * k, 2 * k + 1, 40, 10) for k in range(128)] + [link(255, 256)]
    assert len(rows) == 257
    got = check([rows], [257], st, pa, 'N = cap = 257')
    assert got['group_id'][0, 256] == 254 and got['links'][0] == 129 and got['size_tracks'][0, 3] == 3


@pytest.mark.parametrize('order', ['descending', 'shuffled', 'ascending'])
def test_chain_over_all_slots(order):
    """k - (k + 1) over N = 300 slots: the case that needs many sweeps and the pointer jumping"""
    N = 300
    st, pa = tracks(N, seed=2)
    rows = [link(k, k + 1) for k in range(N - 1)]
    if order == 'descending':
        rows = rows[::-1]
    elif order == 'shuffled':
        rows = [rows[k] for k in np.random.default_rng(5).permutation(N - 1)]
    got = check([rows], [N - 1], st, pa, f'chain {order}')
    assert (got['group_id'] == 0).all() and got['size_tracks'][0, 8] == N and got['links'][0] == N - 1


def test_star_and_two_components_a_failed_candidate_does_not_join():
    N = 40
    st, pa = tracks(N, seed=3)
    star = [link(17, k) for k in range(N // 2) if k != 17]                       # hub 17, leaves 0 .. 19: root 0
    other = [link(k, k + 1) for k in range(20, 29)]                              # 20 .. 29
    bridge = [[5, 25, 1024, 818]]                                                # a candidate one together frame short of a link
    got = check([star + bridge + other], [len(star) + 1 + len(other)], st, pa, 'star + chain + failed bridge')
    gid = got['group_id'][0]
    assert (gid[:20] == 0).all() and (gid[20:30] == 20).all() and gid[30:].tolist() == list(range(30, 40))
    assert got['links'][0] == len(star) + len(other) and got['candidates'][0] == got['links'][0] + 1
    # exactly at near 1024 == share_q co the candidate IS a link, and the two become one
    got = check([star + [[5, 25, 1024, 819]] + other], [len(star) + 1 + len(other)], st, pa, 'bridge at the boundary')
    assert (got['group_id'][0, :30] == 0).all() and got['size_tracks'][0, 8] == 30
    for near, joined in ((2 ** 21 - 1, False), (2 ** 21, True)):                 # the products pass 2^31: 64-bit integers
        got = check([[[0, 1, 2 ** 21, near]]], [1], *tracks(2), 'large counts', share_q=1024)
        assert (got['group_id'][0, 1] == 0) == joined


def test_saturated_sizes_and_an_ineligible_track():
    N = 32
    st, pa = tracks(N, seed=4)
    st[0, 30] = 9                                                                # min_frames - 1: isolated and ineligible
    nine = [link(k, k + 1) for k in range(0, 8)]                                 # 0 .. 8
    twelve = [link(10, k) for k in range(11, 22)]                                # 10 .. 21
    got = check([nine + twelve], [len(nine) + len(twelve)], st, pa, 'groups of 9 and 12')
    assert got['size_tracks'][0].tolist() == [0, N - 22, 0, 0, 0, 0, 0, 0, 21]   # both saturate index g_max; 30 is absent
    assert got['group_id'][0, 30] == -1 and got['size_steps'][0].sum() == st.sum() - 9
    assert got['size_path'][0, 8] == pa[0, :9].sum() + pa[0, 10:22].sum()
    got = check([nine + twelve], [len(nine) + len(twelve)], st, pa, 'g_max = 10', g_max=10)
    assert got['size_tracks'].shape == (1, 11) and got['size_tracks'][0, 9] == 9 and got['size_tracks'][0, 10] == 12
    # an ineligible track inside a component (hand-made rows only; pass 1 never writes one, and the restatement asserts so):
    # as in the package's host half it carries the component and is not counted
    from piml_amd.groupstats import host_rows
    st[0, 4] = 3
    got = run([nine], [len(nine)], st, pa)
    own = host_rows(dict(edges=np.array([[0, *r] for r in nine]), trk_steps=st, trk_path=pa), 10, Q819)
    assert all(np.array_equal(got[k], own[k]) for k in ROWS)
    assert got['group_id'][0, 4] == -1 and got['group_id'][0, 8] == 0 and got['size_tracks'][0, 8] == 8


def test_row_counts_capacity_and_garbage_past_the_count():
    """S = 3 with 0, 1 and cap rows; a member that lists more candidates than the buffer holds; the rows past the count hold
    garbage -- indices far out of range, which would be followed if they were read"""
    N, cap = 12, 5
    st, pa = tracks(N, S=4, seed=6)
    junk = [2 ** 30, -(2 ** 30), 1, 1]
    rows = np.array([[junk] * cap,
                     [link(3, 7)] + [junk] * (cap - 1),
                     [link(0, 1), link(1, 2), link(8, 9), link(9, 2), link(10, 11, 40, 10)],
                     [link(4, 5), link(5, 6), link(0, 11), link(1, 2, 50, 20), link(6, 7)]], np.int64)
    n = [0, 1, cap, cap + 3]                                                     # the last: three rows were never written
    got = check(rows, n, st, pa, 'row counts')
    assert got['candidates'].tolist() == n and got['links'].tolist() == [0, 1, 4, 4]
    assert got['group_id'][0].tolist() == list(range(N)) and got['group_id'][1, 7] == 3
    assert got['group_id'][2].tolist() == [0, 0, 0, 3, 4, 5, 6, 7, 0, 0, 10, 11]
    assert got['group_id'][3].tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 8, 9, 10, 0]
    # a row whose index is out of range inside the count is no link (nothing is written through it)
    got = run([[link(0, 1), [3, N, 30, 30], [-1, 2, 30, 30]]], [3], st[:1], pa[:1])
    assert got['links'].tolist() == [1] and got['candidates'].tolist() == [3] and got['group_id'][0].tolist() == [0, 0] + list(range(2, N))


@functools.lru_cache(maxsize=None)
def large_case():
    N, L = 65536, 4096
    rng = np.random.default_rng(7)
    st, pa = tracks(N, seed=8)
    st[0, rng.integers(0, N, 500)] = 5                                           # some ineligible tracks (isolated ones too)
    chain_slots = rng.permutation(N)[:L]                                         # a 4096-long chain through scattered slots
    rows = [link(int(a), int(b)) for a, b in zip(chain_slots[:-1], chain_slots[1:])]
    free = np.setdiff1d(np.arange(N), chain_slots)
    pick = rng.permutation(free)[:6000].reshape(-1, 2)                           # 3000 scattered pairs, a third not links
    rows += [link(int(a), int(b), 100, 100 if k % 3 else 50) for k, (a, b) in enumerate(pick)]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    ends = np.concatenate([chain_slots, pick.reshape(-1)])                       # every end of a candidate is eligible
    st[0, ends] = np.maximum(st[0, ends], 10)
    return np.array([rows]), [len(rows)], st, pa, int(chain_slots.min())


def test_large_case():
    rows, n, st, pa, root = large_case()
    got = check(rows, n, st, pa, 'N = 65536')
    assert (got['group_id'][0] == root).sum() == 4096 and got['size_tracks'][0, 8] == 4096 and got['links'][0] == 4095 + 2000


# ---- the whole statistics ----

def _equal(a, b):
    from piml_amd.groupstats import ARRAYS
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x, y)), k
    assert a.options == b.options


@pytest.mark.parametrize('N,S,T', CASES)
def test_whole_statistics_on_planted_tracks(N, S, T):
    from piml_amd.groupstats import group_stats
    P, M, plans, runs = planted_case(N, S, T)
    Pt, Mt = torch.tensor(P, device=DEV), torch.tensor(M, device=DEV)
    for kw, want in runs:
        host, dev = group_stats(Pt, Mt, components='host', **kw), group_stats(Pt, Mt, components='device', **kw)
        _equal(host, dev)
        REF.check(dev, want, f'N={N} S={S} T={T} device')
        if N >= 65:
            assert dev.links.sum() > 0 and dev.size_tracks[:, 2:].sum() > 0


def test_whole_statistics_on_the_recorded_clips():
    from piml_amd.groupstats import group_stats_of_raw
    for name in (GC_CLIP, UCY_CLIP):
        raw, P, M, want = clip_case(name)
        host, dev = group_stats_of_raw(raw, components='host'), group_stats_of_raw(raw, components='device')
        _equal(host, dev)
        REF.check(dev, want, name[:3])
        assert dev.links[0] >= 1 and dev.groups(0) == host.groups(0)
    with pytest.raises(ValueError, match=r'max_edges'):                          # the capacity check stays where it was
        group_stats_of_raw(clip_case(GC_CLIP)[0], components='device', max_edges=1)


def test_two_runs_are_equal_and_a_graph_replay_writes_everything():
    from piml_amd import ops_metrics
    rows, n, st, pa, _ = large_case()
    a, b = run(rows, n, st, pa), run(rows, n, st, pa)
    assert all(np.array_equal(a[k], b[k]) for k in ROWS + ('status',))
    N = 300
    st, pa = tracks(N, S=2, seed=9)
    chain = [link(k, k + 1) for k in range(N - 1)][::-1]
    e = np.array([chain, [link(0, 7)] + [link(k, (k + 13) % N, 50, 20 + k % 30) for k in range(1, N - 1)]])
    args = (torch.tensor(e, dtype=torch.int32, device=DEV), torch.tensor([N - 1, N - 1], dtype=torch.int32, device=DEV),
            torch.tensor(st, device=DEV), torch.tensor(pa, device=DEV), 10, Q819)
    eager = ops_metrics.group_components_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.group_components_frames(*args)                               # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.group_components_frames(*args)
    for v in cap.values():
        v.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    for k in ROWS + ('status',):
        assert torch.equal(eager[k], cap[k]), k
        assert k == 'group_id' or not bool((cap[k] == SENTINEL).any()), k        # (-7 is no group_id either: >= -1)
    assert int(cap['group_id'].min()) >= -1
    want = want_of(e, [N - 1, N - 1], st, pa)
    assert all(np.array_equal(cap[k].cpu().numpy(), want[k]) for k in ROWS)


# ---- the group side of the statistics fit ----

FRAMES, FIT_SEEDS, MIN_COUNT = 60, [0, 1], 5
MIN_TIME = 12.5 * 0.08                        # min_time scaled to the short window: min_frames = 13


GDIST = 0.25                                  # a pair planted 0.8 m apart is 0.4 m from its centroid: the term is felt at 0.25,
#                                               and moves the member distances of every planted unit


def _scene():
    from test_scenario_groups_gpu import scene
    return scene()


def _law():
    from test_scenario_groups_gpu import NO_PAIRS
    return dict(NO_PAIRS)


@functools.lru_cache(maxsize=None)
def reference_groups():
    """the pooled GroupStats of three other seeds under Ag = 3 (made once, left unchanged)"""
    from piml_amd.models.mlapm import MLAPM
    ens = MLAPM(**_law(), Ag=3.0, group_dist=GDIST).simulate_ensemble(_scene(), FRAMES, [7, 8, 9])
    return ens.group_stats(min_time=MIN_TIME).pooled()


def test_evaluator_terms_are_stats_objective_by_hand():
    from piml_amd.calibrate import OBJECTIVE_KEYS, _StatsEvaluator, stats_objective
    from piml_amd.models.mlapm import MLAPM
    ref = reference_groups()
    cands = [dict(_law(), Ag=0.0, group_dist=GDIST), dict(_law(), Ag=3.0, group_dist=GDIST)]
    ev = _StatsEvaluator(_scene(), (None, None, None, ref), FRAMES, FIT_SEEDS, len(cands), 0.3, None, None, None, None,
                         MIN_COUNT, DEV)
    assert ev.group_kw['min_time'] == MIN_TIME and set(ev.group_kw) == {'radius', 'dv_max', 'v_min', 'min_time', 'share',
                                                                       'r_bin', 'r_bins', 'a_bins'}
    J = ev(cands)
    assert ev.seconds['groups'] > 0
    sw = MLAPM.simulate_sweep(_scene(), FRAMES, cands, FIT_SEEDS)
    st = sw.group_stats(min_time=MIN_TIME, components='host')
    for c in range(len(cands)):
        mine = st.select(sw.members_of(c)).pooled()
        assert mine.links[0] >= 1, f'candidate {c}: the simulated side holds no link'
        Jh, terms = stats_objective(groups=mine, ref_groups=ref, min_count=MIN_COUNT)
        print(f'\n[group fit] Ag = {cands[c]["Ag"]}: J = {Jh:.4f}, terms {terms}, links {int(mine.links[0])}')
        assert ev.last_terms[c].keys() == terms.keys()
        for k in OBJECTIVE_KEYS['groups']:
            a, b = ev.last_terms[c][k], terms[k]
            assert a == b or (np.isnan(a) and np.isnan(b)), (c, k, a, b)
        assert J[c] == Jh and np.isfinite(Jh)
        assert all(np.isfinite(terms[k]) for k in OBJECTIVE_KEYS['groups'][:4]), terms       # every weighted term
    a, b = ev.last_terms
    assert a['group_fraction_diff'] != b['group_fraction_diff'] or a['member_distance_l1'] != b['member_distance_l1']


def test_tiny_fit_of_the_group_term():
    from piml_amd.calibrate import calibrate_mlapm_to_stats
    from piml_amd.models.mlapm import DEFAULT_GROUP_DIST, MLAPM
    law = {k: v for k, v in _law().items() if k != 'version'}
    kw = dict(version='GC', init={**law, 'Ag': 1.0, 'group_dist': GDIST}, fit=('Ag',), frames=FRAMES, population=4, generations=2, seeds=range(2),
              min_count=MIN_COUNT)
    ref = (None, None, None, reference_groups())
    a = calibrate_mlapm_to_stats(_scene(), ref, **kw)
    assert all(y <= x for x, y in zip(a.history, a.history[1:])) and len(a.history) == 2 and np.isfinite(a.final_loss)
    assert a.params['Ag'] >= 0 and a.params['group_dist'] == GDIST != DEFAULT_GROUP_DIST and a.status == 'ok'
    assert a.seconds['groups'] > 0 and set(a.terms) >= {'group_fraction_diff', 'size_l1', 'member_distance_l1', 'abreast_l1'}
    b = calibrate_mlapm_to_stats(_scene(), ref, **kw)
    assert a.params == b.params and a.history == b.history
    MLAPM(**a.params)                                                            # the result is a law as it stands
