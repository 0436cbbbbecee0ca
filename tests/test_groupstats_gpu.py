"""GPU: group statistics (piml_group_pairs, piml_group_members, piml_amd.groupstats) against the numpy restatement
(groupstats_ref.py) on planted tracks, the analytic scene and the recorded GC and UCY clips; the edge overflow; determinism
(two calls, graph replay of pass 1, member against a one-member call, a permutation of the slots), a short GC ensemble
against its members and the two command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import groupstats_ref as REF
from conftest import GOLDEN, REPO
from test_groupstats import CASES, GC_CLIP, TILE, UCY_CLIP, assert_cap, clip_case, planted_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Q = REF.Q
SEEDS, FRAMES = [0, 1, 2], 40                 # the short GC ensemble
MIN_TIME = 12.5 * 0.08                        # min_time scaled to its 40 frames: min_frames = 13


def _gpu(*xs):
    return [torch.tensor(np.asarray(x), device=DEV) for x in xs]


def _bits_equal(a, b, names=None):
    from piml_amd.groupstats import ARRAYS
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names or ARRAYS)


def check_identities(st):
    near_links = np.zeros(st.members, np.int64)
    link = st.edges[:, 4] * 1024 >= st.options['share_q'] * st.edges[:, 3]
    np.add.at(near_links, st.edges[link, 0], st.edges[link, 4])
    assert np.array_equal(st.dist.sum(-1), st.link_frames) and np.array_equal(st.link_frames, near_links)
    assert np.array_equal(st.abreast.sum(-1) + st.abreast_skipped, st.link_frames)
    assert np.array_equal(st.size_tracks.sum(-1), (st.trk_steps >= st.options['min_frames']).sum(-1))
    assert np.array_equal(st.size_steps.sum(-1), np.where(st.group_id >= 0, st.trk_steps, 0).sum(-1))
    assert np.array_equal(st.n_edges, st.candidates) and (st.together <= st.pairs).all() and (st.size_tracks[:, 0] == 0).all()


@pytest.mark.parametrize('N,S,T', CASES)
def test_planted_tracks_against_numpy(N, S, T):
    from piml_amd.groupstats import group_stats
    from piml_amd.trackstats import track_stats
    P, M, plans, runs = planted_case(N, S, T)
    Pt, Mt = _gpu(P, M)
    for kw, want in runs:
        label = f'N={N} S={S} T={T} {sorted(kw)}'
        assert_cap(want, label)                                  # on the restatement alone, before the device is looked at
        st = group_stats(Pt, Mt, **kw)
        REF.check(st, want, label)
        check_identities(st)
        assert st.pairs.sum() == want['n_items']
        if T >= 2:
            tk = {k: kw[k] for k in ('dt', 'frames', 'n_active') if k in kw}
            ts = track_stats(Pt, Mt, n_lags=1, **tk)
            assert np.array_equal(st.trk_steps, ts.trk_steps) and np.array_equal(st.trk_path, ts.trk_path)
        if N >= 65:                                              # no output is vacuous
            assert st.links.sum() > 0 and any(len(g) == 3 for m in range(S) for g in st.groups(m))
            assert st.dist.sum() > 0 and st.abreast.sum() > 0 and st.size_tracks[:, 2:].sum() > 0 and st.dist_sum.sum() > 0
            assert st.candidates.sum() > st.links.sum() and st.size_tracks[:, 1].sum() > 0
    kw, want = runs[0]
    st = group_stats(Pt, Mt, **kw)
    if N == 1:
        assert all(np.abs(getattr(st, k)).sum() == 0 for k in REF.PAIR_ROWS + REF.MEMBER_ROWS) and st.edges.shape == (0, 5)
        assert (st.group_id == -1).all()
    if N == 2:                                                   # one pair-frame, one link
        assert st.edges.tolist() == [[0, 0, 1, 1, 1]] and st.links.tolist() == [1] and st.pairs.tolist() == [1]
        assert st.groups(0) == [[0, 1]] and st.link_frames.tolist() == [1]
    if N == 3:                                                   # every track spans more than two staged tiles
        there = np.nonzero(REF.participants(P[0], M[0]).all(-1))[0]
        assert there[-1] - there[0] > 2 * TILE and st.trk_steps.min() > TILE and st.edges[:, 3].min() > TILE
        assert st.groups(0) == [[0, 1, 2]]


def test_analytic_scene_is_exact():
    """the hand-counted scene of test_groupstats.py on the device: hand counts == device == both restatements"""
    from piml_amd.groupstats import group_stats
    P, M, kw, hand = REF.analytic_scene()
    st = group_stats(*_gpu(P, M), **kw)
    ref = REF.group_stats(P, M, **kw)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(st, k), hand[k]), (k, getattr(st, k), hand[k])
        assert np.array_equal(ref[k], hand[k]) and np.array_equal(ref['f64'][k], hand[k]), k
    assert st.groups(0) == [[0, 1, 2]] and st.links[0] == 3 and st.group_id[0, 3:].tolist() == [3, 4, 5]
    assert st.abreast[0, 0] == 39 and st.abreast[0, -1] == 39 and st.abreast[0].sum() == 3 * 39        # 0-1 abreast, 0-2 in file
    assert np.nonzero(st.dist[0])[0].tolist() == [8, 12, 14]                                         # 1 m, 1.5 m, sqrt(3.25) m
    dt = float(np.float32(0.08))
    speed = st.speed_by_size()
    assert speed[3] == (3 * 39 * (Q // 8)) / float(Q) / dt / (3 * 39) and speed[1] == (2 * 39 * (Q // 8)) / float(Q) / dt / (3 * 39)
    assert st.group_fraction() == 0.5 and st.speed_ratio() == pytest.approx(1.5)


def test_edge_overflow_names_the_count_needed():
    from piml_amd.groupstats import group_stats
    P, M, plans, runs = planted_case(65, 3, 40)
    kw, want = runs[0]
    need = int(want['n_edges'].max())
    assert need >= 2
    Pt, Mt = _gpu(P, M)
    with pytest.raises(ValueError, match=rf'\b{need}\b'):
        group_stats(Pt, Mt, max_edges=1, **kw)
    REF.check(group_stats(Pt, Mt, max_edges=need, **kw), want, 'max_edges = the count needed')


def test_determinism_graph_members_and_slot_permutation():
    from piml_amd import ops_metrics
    from piml_amd.groupstats import ADDITIVE, group_stats
    P, M, plans, runs = planted_case(65, 3, 40)
    S, T, N = M.shape
    Pt, Mt = _gpu(P, M)
    kw = dict(frames=(2, T - 1), min_time=9.5 * 0.08, radius=1.8, a_bins=7)
    a, b = group_stats(Pt, Mt, **kw), group_stats(Pt, Mt, **kw)
    assert _bits_equal(a, b) and a.links.min() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), group_stats(Pt[m], Mt[m], **kw)), m
    # a permutation of the slots: the groups map through it, every additive row stays
    perm = np.random.default_rng(0).permutation(N)               # new slot k holds old slot perm[k]
    inv = np.argsort(perm)
    c = group_stats(Pt[:, :, perm], Mt[:, :, perm], **kw)
    assert _bits_equal(a, c, ADDITIVE)
    assert np.array_equal(c.trk_steps, a.trk_steps[:, perm]) and np.array_equal(c.trk_path, a.trk_path[:, perm])
    for m in range(S):
        assert sorted(sorted(int(inv[x]) for x in g) for g in a.groups(m)) == sorted(c.groups(m)), m
        rows = a.edges[a.edges[:, 0] == m]
        mapped = sorted((min(inv[i], inv[j]), max(inv[i], inv[j]), co, near) for _, i, j, co, near in rows.tolist())
        assert mapped == [tuple(r) for r in c.edges[c.edges[:, 0] == m][:, 1:].tolist()], m
    # pass 1 replayed from a graph (the whole operator reads the candidate counts back between its passes)
    r2, dv2, vm2, min_frames, _ = ops_metrics.group_thresholds(0.08, 1.8, 0.5, 0.1, kw['min_time'], 0.8)
    args = (Pt, Mt, r2, dv2, vm2, min_frames, kw['frames'], None, 64)
    eager = ops_metrics.group_pairs_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.group_pairs_frames(*args)                    # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.group_pairs_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k in ('n_edges',) + ops_metrics.GROUP_PAIR_ROWS:
        assert torch.equal(eager[k], cap[k]), k
        assert np.array_equal(eager[k].cpu().numpy(), getattr(a, k)), k
    for m in range(S):
        n = int(eager['n_edges'][m])
        rows = [sorted(x['edges'][m, :n].cpu().numpy().tolist()) for x in (eager, cap)]
        assert rows[0] == rows[1] == a.edges[a.edges[:, 0] == m][:, 1:].tolist(), m


def test_recorded_clips():
    from piml_amd.groupstats import compare_group_stats, group_stats_of_raw
    out = {}
    for name in (GC_CLIP, UCY_CLIP):
        raw, P, M, want = clip_case(name)
        assert_cap(want, name[:3])
        st = group_stats_of_raw(raw)
        assert st.options['dt'] == float(raw.time_unit)
        REF.check(st, want, name[:3])
        check_identities(st)
        assert st.links[0] >= 1 and st.groups(0)
        out[name] = st
        print(f'[groupstats] {name[:3]}: {st.eligible_tracks()} eligible tracks, {int(st.links[0])} links, groups {st.groups(0)}, '
              f'group fraction {st.group_fraction():.3f}, speed by size {np.round(st.speed_by_size()[1:4], 3).tolist()} m/s, mean '
              f'member distance {st.mean_member_distance():.3f} m')
    cmp = compare_group_stats(out[GC_CLIP], out[UCY_CLIP], min_count=5)
    print(f'[groupstats] GC vs UCY: {cmp}')
    assert all(np.isfinite(v) for v in cmp.values()), cmp
    assert cmp == compare_group_stats(group_stats_of_raw(clip_case(GC_CLIP)[0]), group_stats_of_raw(clip_case(UCY_CLIP)[0]), min_count=5)


@pytest.fixture(scope='module')
def gc_ensemble():
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    from piml_amd.simulate import load_mlapm_params
    return MLAPM(**load_mlapm_params(None)).simulate_ensemble(gc_scenario().to(DEV), FRAMES, SEEDS)


def test_short_ensemble_against_members_and_numpy(gc_ensemble):
    from piml_amd.groupstats import ADDITIVE, group_stats_of_raw
    ens = gc_ensemble
    st = ens.group_stats(min_time=MIN_TIME)
    assert st.members == len(SEEDS) and st.options['dt'] == float(ens.time_unit) and st.options['min_frames'] == 13
    assert st.pairs.sum() > 0 and (st.slices == FRAMES).all()
    for m in range(len(SEEDS)):
        mem = ens.member(m)
        one = mem.group_stats(min_time=MIN_TIME)
        assert _bits_equal(st.member(m), one), m
        raw = group_stats_of_raw(mem.to_raw_data(), min_time=MIN_TIME)       # the clip holds the member's num_agents slots only
        n = mem.num_agents
        assert _bits_equal(one, raw, ADDITIVE + ('edges', 'n_edges')), m
        for k in ('trk_steps', 'trk_path', 'group_id'):
            assert np.array_equal(getattr(one, k)[:, :n], getattr(raw, k)), (m, k)
    cap = ens.position.shape[2]
    want = REF.group_stats(ens.position.cpu().numpy(), ens.mask_p.cpu().numpy(), n_active=[min(n, cap) for n in ens.spawned],
                           dt=float(ens.time_unit), min_time=MIN_TIME)
    assert_cap(want, 'MLAPM GC ensemble')
    REF.check(st, want, 'MLAPM GC ensemble')
    check_identities(st)


def test_command_lines(tmp_path, gc_ensemble):
    """`simulate --group-stats` and `python -m piml_amd.groupstats --data ... --ref ...` in child processes write what the
    Python calls return"""
    from piml_amd.crowdstats import _load
    from piml_amd.groupstats import ADDITIVE, GroupStats, group_stats_of_raw, merge
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'groups.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scenario', 'gc', '--seeds', '0:3',
                        '--frames', str(FRAMES), '--out', clip, '--group-stats', out], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = GroupStats.from_json(out)
    own = gc_ensemble.group_stats()
    assert _bits_equal(st, own), 'the JSON of the command line differs from the in-process statistics'
    assert st.options == own.options and not os.path.exists(clip.replace('{seed}', '0'))
    assert '[groupstats] simulate --group-stats' in p.stdout
    # the stand-alone command on clips the ensemble wrote, against the recorded clip
    paths = gc_ensemble.save_data(clip)
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    cli = str(tmp_path / 'cli.json')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.groupstats', '--data', *paths, '--ref', ref, '--frames', f'0:{FRAMES}',
                        '--min-time', '1.0', '--radius', '1.5', '--out', cli], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(cli) as fh:
        d = json.load(fh)
    data, rs = GroupStats.from_json(d['data']), GroupStats.from_json(d['ref'])
    kw = dict(frames=(0, FRAMES), min_time=1.0, radius=1.5)
    assert data.edges is None and rs.edges is not None and data.options['radius'] == 1.5 and rs.options['min_frames'] == 13
    assert _bits_equal(data, merge([group_stats_of_raw(_load(q), **kw) for q in paths]), ADDITIVE)
    assert _bits_equal(rs, group_stats_of_raw(_load(ref), **kw))
    assert set(d['compare']) == {'group_fraction_diff', 'size_l1', 'member_distance_l1', 'abreast_l1', 'speed_ratio_diff'}
    assert 'data vs ref' in p.stdout and 'eligible tracks' in p.stdout
