"""GPU: heading-frame pair statistics (piml_view_stats, piml_amd.viewstats) against the numpy restatement (viewstats_ref.py)
on random slices, an analytic scene with hand counts, its quarter turn and a nearest-neighbour tie, the recorded GC and UCY
clips; determinism (two calls, graph replay, member against a one-member call); runs of slices (run = 3 against the
restatement, run = VS_MAX_RUN bit for bit against run = 1); ensembles against their members, the two command lines, and one
generation of the statistics fit with a view side.  The inputs and their restatements are in viewstats_shapes.py; that at
most CAP of their pairs are ambiguous is checked on the CPU by test_viewstats.py and again here."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import viewstats_ref as REF
import viewstats_shapes as SH
from conftest import GOLDEN, REPO
from test_pairstats_gpu import _gpu, _raw, sim  # noqa: F401  (sim: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G0, GB0 = 24, 60                              # the default map side and gap bins


def _checked(st, want, label):
    share = SH.ambiguous_share(want)
    print(f'\n[viewstats] {label}: {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous ({share:.2e})')
    assert share <= SH.CAP, share
    REF.check(st, want, label)


def _bits_equal(a, b):
    return all(np.array_equal(getattr(a, k), b[k] if isinstance(b, dict) else getattr(b, k)) for k in REF.OUTPUTS)


def _derived(st, tag):
    side, chance = st.passing_side()
    m, s = st.headway_fit()
    print(f'[viewstats] {tag}: front/back ratio {st.front_back_ratio():.4f}, passing side {side:+.4f} (chance {chance:+.4f}), '
          f'mean front gap {st.mean_front_gap():.3f} m, headway fit {m:.3f} m + {s:.3f} s x speed')


@pytest.mark.parametrize('N,S,T', SH.CASES)
def test_random_slices_against_numpy(N, S, T):
    from piml_amd.viewstats import view_stats
    P, V, M, _ = SH.case_inputs(N, S, T)
    Pt, Vt, Mt = _gpu(P, V, M)
    for which, kw in enumerate(SH.option_sets(N, S, T)):
        st = view_stats(Pt, Vt, Mt, **kw)
        _checked(st, SH.case_reference(N, S, T, which), f'N={N} S={S} T={T} {sorted(kw)}')
        assert st.nn_map.sum() == st.focal[:, 0].sum() == st.front_gap.sum()
        assert st.map.sum() <= st.pairs.sum()
        if N >= 300:                               # not vacuous: every class, a front gap and a nearest neighbour on the map
            a, b = kw.get('frames', (0, T))            # (every class of every lag that has a slice in the window)
            live = [k for k, lag in enumerate((0,) + tuple(kw['lags'])) if lag < b - a]
            assert (st.map.sum((0, 3, 4))[live] > 0).all() and st.front_gap[:, :-1].sum() > 0 and st.nn_map[:, :-1].sum() > 0
            assert st.front_speed.sum() > 0
        if 'n_active' in kw and S > 1:             # the member without a slot: nothing
            assert all((getattr(st, k)[S // 2] == 0).all() for k in REF.OUTPUTS)
    if N == 1:                                     # nobody to pair: every focal agent in the last bins
        assert st.pairs.sum() == 0 and st.map.sum() == 0 and st.focal[:, 0].sum() > 0
        assert st.nn_map[:, -1].sum() == st.focal[:, 0].sum() == st.front_gap[:, -1].sum() and st.front_speed.sum() == 0


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene

def _hand_counts(P, V, focal_only=None):
    """the counts of one frame with the default options, every step written out in Python floats"""
    n = len(P)
    out = dict(focal=0, pairs=0, map=np.zeros((4, G0, G0), np.int64), nn_map=np.zeros(G0 * G0 + 1, np.int64),
               front_gap=np.zeros(GB0 + 1, np.int64), front_speed=np.zeros(GB0, np.int64))
    cs = float(REF.COS_SAME)
    for i in range(n):
        sp = math.hypot(*V[i])
        if sp < 0.1 or (focal_only is not None and i != focal_only):
            continue
        hx, hy = V[i][0] / sp, V[i][1] / sp
        out['focal'] += 1
        nearest, gap = (math.inf, G0 * G0), math.inf
        for j in range(n):
            if j == i:
                continue
            dx, dy = P[j][0] - P[i][0], P[j][1] - P[i][1]
            a, l = dx * hx + dy * hy, dy * hx - dx * hy
            out['pairs'] += 1
            spj = math.hypot(*V[j])
            if spj < 0.1:
                c = 0
            else:
                q = (hx * V[j][0] + hy * V[j][1]) / spj
                c = 1 if q >= cs else 2 if q <= -cs else 3
            cx, cy = math.floor((a + 3.0) / 0.25), math.floor((l + 3.0) / 0.25)
            cell = cy * G0 + cx if 0 <= cx < G0 and 0 <= cy < G0 else G0 * G0
            if cell < G0 * G0:
                out['map'][c, cy, cx] += 1
            if math.hypot(dx, dy) < nearest[0]:
                nearest = (math.hypot(dx, dy), cell)
            if a > 0 and abs(l) < 0.4:
                gap = min(gap, a)
        out['nn_map'][nearest[1]] += 1
        b = min(math.floor(gap / 0.1), GB0) if math.isfinite(gap) else GB0
        out['front_gap'][b] += 1
        if b < GB0:
            out['front_speed'][b] += int(np.rint(np.float32(np.sqrt(np.float32(V[i][0]) ** 2 + np.float32(V[i][1]) ** 2))
                                                 * np.float32(1 << 20)))
    return out


def _equals_hand(st, hand):
    return all(np.array_equal(np.asarray(st[k] if isinstance(st, dict) else getattr(st, k))[0].reshape(-1),
                              np.asarray(hand[k]).reshape(-1)) for k in REF.OUTPUTS)


def _scene():
    P, V = np.array(SH.SCENE_P, np.float32)[None], np.array(SH.SCENE_V, np.float32)[None]
    return P, V, np.ones((1, P.shape[1]), np.float32)


def test_analytic_scene_hand_counts_and_quarter_turn():
    from piml_amd.viewstats import Q, view_stats
    P, V, M = _scene()
    speed0 = int(np.rint(np.float32(1.3) * np.float32(Q)))
    # the agent at the origin alone as the focal one (a box around it): every count by hand
    st = view_stats(*_gpu(P, V, M), lags=(), box=(-0.5, 0.5, -0.5, 0.5))
    want = np.zeros((4, G0, G0), np.int64)
    want[2, 13, 20] = 1                            # 1: oncoming at 2.06 ahead, 0.29 left
    want[1, 12, 15] = 1                            # 2: with, 0.93 ahead, 0.17 left
    want[1, 11, 19] = 1                            # 3: with, 1.77 ahead, 0.18 right
    want[0, 14, 6] = 1                             # 4: standing, 1.28 behind, 0.52 left
    want[3, 5, 13] = 1                             # 5: crossing, 0.34 ahead, 1.54 right
    assert st.focal.tolist() == [[1]] and st.pairs.tolist() == [[5]] and np.array_equal(st.map[0, 0], want)
    assert st.nn_map[0, 12 * G0 + 15] == 1 and st.nn_map.sum() == 1            # 2 is the nearest, at 0.945 m
    assert st.front_gap[0, 9] == 1 and st.front_gap.sum() == 1                # 0.93 m in the corridor; 1 and 3 are further
    assert st.front_speed[0, 9] == speed0 == 1363149 and st.front_speed.sum() == speed0
    assert _equals_hand(st, _hand_counts(SH.SCENE_P, SH.SCENE_V, 0))
    # every mover in turn as the focal one: the standing agent 4 is a source only
    full = view_stats(*_gpu(P, V, M), lags=())
    hand = _hand_counts(SH.SCENE_P, SH.SCENE_V)
    assert full.focal.tolist() == [[5]] and full.pairs.tolist() == [[25]] and hand['map'].sum() > 15
    assert _equals_hand(full, hand)
    assert (full.map[0, 0] >= want).all() and full.front_gap[0, 9] >= 1
    ref = REF.view_stats(P, V, M, lags=())
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(full, k), ref[k]) and np.array_equal(getattr(full, k), ref['f32'][k]), k
    # the scene turned by 90 degrees, velocities with it: the heading frame turns along, nothing changes
    turned = view_stats(*_gpu(SH.rotate(P), SH.rotate(V), M), lags=())
    assert _bits_equal(turned, full)
    assert _bits_equal(view_stats(*_gpu(SH.rotate(P), SH.rotate(V), M), lags=(), box=(-0.5, 0.5, -0.5, 0.5)), st)


def test_nearest_neighbour_tie_goes_to_the_lowest_slot():
    """two standing sources at exactly the same distance (dx and dy exchanged: the same float32 sum), in different cells"""
    from piml_amd.viewstats import view_stats
    V = np.array([[1.3, 0.0], [0.0, 0.0], [0.0, 0.0]], np.float32)[None]
    M = np.ones((1, 3), np.float32)
    a, b = [0.45, 1.15], [1.15, 0.45]             # neither in the corridor: 0.45 m to the side
    cell = lambda p: int(math.floor((p[1] + 3.0) / 0.25)) * G0 + int(math.floor((p[0] + 3.0) / 0.25))   # noqa: E731
    assert cell(a) != cell(b)
    for first, second in ((a, b), (b, a)):
        P = np.array([[0.0, 0.0], first, second], np.float32)[None]
        d = P[0, 1:] - P[0, 0]
        assert np.sqrt(d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1]) == np.sqrt(d[1, 0] * d[1, 0] + d[1, 1] * d[1, 1])
        st = view_stats(*_gpu(P, V, M), lags=())
        assert st.focal.tolist() == [[1]] and st.nn_map[0, cell(first)] == 1 and st.nn_map.sum() == 1
        assert st.map[0, 0, 0].sum() == 2 and st.front_gap[0, -1] == 1


# ---------------------------------------------------------------------------------------------------------------------
# determinism

def _replayed(fn, *args, **kw):
    """fn's outputs eagerly and from a captured graph replayed twice"""
    eager = fn(*args, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(*args, **kw)                                          # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = fn(*args, **kw)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    return eager, cap


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.viewstats import view_stats
    from test_flowstats_gpu import flow_slices
    S, T, N = 3, 30, 400
    P, V, M, side = flow_slices(S, T, N, seed=11)
    Pt, Vt, Mt = _gpu(P, V, M)
    kw = dict(lags=(3, 7, 20), box=(0.0, side * 0.7, 0.0, side * 0.7))
    a, b = view_stats(Pt, Vt, Mt, **kw), view_stats(Pt, Vt, Mt, **kw)
    assert _bits_equal(a, b) and a.map.sum() > 0 and a.front_speed.sum() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), view_stats(Pt[m], Vt[m], Mt[m], **kw)), m
    eager, cap = _replayed(ops_metrics.view_stats_frames, Pt, Vt, Mt, lags=kw['lags'], box=kw['box'])
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


# ---------------------------------------------------------------------------------------------------------------------
# runs of slices

def _distinct(rows):
    return len({np.ascontiguousarray(r).tobytes() for r in rows}) == len(rows)


@pytest.mark.parametrize('name,variant', SH.MID_CALLS)
def test_run3_against_numpy(name, variant):
    from piml_amd.viewstats import view_stats
    c = SH.MID[name]
    SH.check_run_shapes()
    S, T, lags = c['S'], c['T'], c['lags']
    assert SH.run_of(S, T, lags) == 3 and SH.offsets(T, lags)[-1] % 3 != 0
    assert SH.member_boundaries_inside_runs(S, T, lags)                       # member and lag boundaries inside runs
    assert {k for _, k in SH.lag_boundaries_inside_runs(S, T, lags)} == {1, 2}
    P, V, M, _ = SH.mid_inputs(name)
    kw = SH.mid_options(name, variant)
    st = view_stats(*_gpu(P, V, M), **kw)
    _checked(st, SH.mid_reference(name, variant), f'run 3, {name} {variant}')
    bound = kw.get('n_active', [c['N']] * S)
    full = [s for s in range(S) if bound[s] >= 2]
    for s in full:                                                            # no member's statistics are vacuous
        for k in (0, 1, 2):
            assert st.focal[s, k] > 0 and st.pairs[s, k] > 0 and (st.map[s, k].sum((1, 2)) > 0).all(), (s, k)
        assert st.nn_map[s].sum() == st.focal[s, 0] == st.front_gap[s].sum() and st.front_gap[s, :-1].sum() > 0
        assert _distinct([st.map[s, k] for k in (0, 1, 2)]), s
    for k in ('map', 'nn_map', 'front_gap', 'front_speed'):
        assert _distinct([getattr(st, k)[s] for s in full]), k
    if len(lags) == 3:                                                        # the lag past the window: no slices
        assert all((getattr(st, k)[:, 3] == 0).all() for k in ('focal', 'pairs', 'map'))
    if variant == 'n_active':
        empty = [s for s in range(S) if bound[s] == 0]
        assert len(empty) == 1 and all((getattr(st, k)[empty[0]] == 0).all() for k in REF.OUTPUTS)
        assert st.focal[4, 0] < st.focal[3, 0] * 0.7                          # half the slots


def test_run64_equals_run1_bit_for_bit():
    from piml_amd.viewstats import view_stats
    from test_flowstats_gpu import flow_slices
    c = SH.LONG
    SH.check_run_shapes()
    assert SH.run_of(c['S'], c['T'], c['lags']) == SH.constant('VS_MAX_RUN') == c['run']
    P, V, M, side = flow_slices(c['S'], c['T'], c['N'], seed=c['seed'])
    Pt, Vt, Mt = _gpu(P, V, M)
    kw = dict(lags=c['lags'], box=(0.0, 0.8 * side, 0.0, 0.8 * side), **SH.WIDE)
    st = view_stats(Pt, Vt, Mt, **kw)
    for s in range(c['S']):
        assert all(st.map[s, k].sum() > 0 for k in (0, 1, 2)) and st.focal[s, 3] == 0 and st.front_gap[s, :-1].sum() > 0, s
    assert _distinct(list(st.map)) and _distinct(list(st.nn_map)) and _distinct(list(st.front_speed))
    g = SH.run_one_group(c['T'], c['lags'])
    for a in range(0, c['S'], g):
        b = min(a + g, c['S'])
        assert SH.run_of(b - a, c['T'], c['lags']) == 1
        part = view_stats(Pt[a:b], Vt[a:b], Mt[a:b], **kw)
        for k in REF.OUTPUTS:
            assert np.array_equal(getattr(st, k)[a:b], getattr(part, k)), (k, a, b)
    assert _bits_equal(st, view_stats(Pt, Vt, Mt, **kw))


# ---------------------------------------------------------------------------------------------------------------------
# recorded clips, simulated ensembles, command lines, the fit

def test_recorded_clips():
    from piml_amd.viewstats import compare_view_stats, view_stats_of_raw
    out = {}
    for name, box in SH.CLIPS:
        st = view_stats_of_raw(_raw(name), box=box)
        _checked(st, SH.clip_reference(name, box), name)
        assert st.focal[0, 0] > 0 and st.map[0, 0].sum() > 0 and st.map[0, 1:].sum() > 0 and st.front_gap[0, :-1].sum() > 0
        out[name] = st
        _derived(st, name)
    c = compare_view_stats(out[SH.GC_CLIP], out[SH.UCY_CLIP], min_count=20)
    assert c == compare_view_stats(out[SH.GC_CLIP], out[SH.UCY_CLIP], min_count=20)
    assert np.isfinite(c['map_l1']) and np.isfinite(c['nn_map_l1']) and np.isfinite(c['gap_l1'])
    assert np.isfinite(c['front_back_diff']) and np.isfinite(c['passing_side_diff'])


def test_simulated_ensembles(sim):
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.viewstats import view_stats_of_raw
    sc = SCENARIOS['gc']().to(DEV)
    kw = dict(lags=(8, 24), box=SH.GC_BOX)
    ens = sim.simulate_ensemble(sc, 100, [0, 1, 2])
    st = ens.view_stats(**kw)
    assert st.focal.shape == (3, 3) and st.map.shape == (3, 3, 4, G0, G0) and st.pairs[:, 0].sum() > 0
    for m in range(3):
        mem = ens.member(m)
        one = mem.view_stats(**kw)
        assert _bits_equal(st.member(m), one), m
        assert _bits_equal(one, view_stats_of_raw(mem.to_raw_data(), **kw)), m
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    cw = SCENARIOS['crosswalk']().to(DEV)
    me = law.simulate_ensemble(cw, 80, [4, 5, 6])
    kw = dict(lags=(8, 24), cell=0.5, half=6, gap_bin=0.25, gap_bins=24)      # wider cells: fewer pairs near an edge
    ms = me.view_stats(**kw)
    for m in range(3):
        mem = me.member(m)
        assert _bits_equal(ms.member(m), mem.view_stats(**kw)), m
        assert _bits_equal(ms.member(m), view_stats_of_raw(mem.to_raw_data(), **kw)), m
    cap = me.position.shape[2]
    want = REF.view_stats(me.position.cpu().numpy(), me.velocity.cpu().numpy(), me.mask_p.cpu().numpy(),
                          n_active=[min(n, cap) for n in me.spawned], **kw)
    _checked(ms, want, 'MLAPM crosswalk ensemble')
    assert ms.map[:, 0, 2].sum() > 0                                         # a crosswalk has oncoming pairs
    _derived(ms, 'MLAPM crosswalk, 3 x 80 frames')


def test_simulate_cli_view_stats(tmp_path):
    from piml_amd.viewstats import ViewStats, compare_view_stats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'views.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:2', '--frames', '40', '--out', clip,
                        '--view-stats', out, '--view-lags', '8,16'], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = ViewStats.from_json(out)
    assert st.focal.shape == (2, 3) and st.options['lags'] == (8, 16) and st.focal.min() > 0 and st.map[:, 1:].sum() > 0
    assert not os.path.exists(clip.replace('{seed}', '0'))
    assert '[viewstats] simulate --view-stats' in p.stdout
    c = compare_view_stats(st, st)
    assert all(v == 0 for k, v in c.items() if k != 'g_map_cells' and np.isfinite(v))


def test_viewstats_cli(tmp_path):
    from piml_amd.viewstats import ViewStats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'cli.json')
    data = os.path.join(GOLDEN, 'data', SH.GC_CLIP + '_simulation.npy')
    ref = os.path.join(GOLDEN, 'data', SH.GC_CLIP + '.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.viewstats', '--data', data, '--ref', ref, '--box', 'auto',
                        '--lags', '16,32', '--out', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(out) as fh:
        d = json.load(fh)
    st, rs = ViewStats.from_json(d['data']), ViewStats.from_json(d['ref'])
    assert st.options['lags'] == (16, 32) == rs.options['lags'] and st.focal[0, 0] > 0 and rs.map.sum() > 0
    assert set(d['compare']) >= {'map_l1', 'nn_map_l1', 'gap_l1', 'front_back_diff', 'passing_side_diff', 'g_map_max_diff',
                                 'headway_slope_diff', 'headway_intercept_diff'}
    assert 'front/back ratio' in p.stdout and 'passing side' in p.stdout and 'headway fit' in p.stdout


def test_one_generation_of_the_fit_with_a_view_side():
    """the plumbing, not identifiability: 1 generation x 4 candidates x 2 seeds x 60 frames of the GC scene against the view
    statistics of a run of the starting law on other seeds"""
    from piml_amd.calibrate import OBJECTIVE_KEYS, calibrate_mlapm_to_stats
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from test_scenario_mlapm_gpu import LAW
    sc = SCENARIOS['gc']().to(DEV)
    frames, kw = 60, dict(lags=(8, 16), cell=1.0, half=8)
    ref = MLAPM(version='GC', **LAW).simulate_ensemble(sc, frames, [7, 8]).view_stats(**kw).pooled()
    assert ref.map[:, 0].sum() > 0 and ref.map[:, 1:].sum() > 0 and ref.map[:, 0, 2].sum() > 0
    res = calibrate_mlapm_to_stats(sc, (None, None, None, None, None, ref), init=dict(LAW), fit=('theta',), frames=frames,
                                   seeds=[0, 1], population=4, generations=1, min_count=1)
    print(f'\n[viewstats] fit: objective {res.initial_loss:.4g} -> {res.final_loss:.4g}; terms {res.terms}')
    assert math.isfinite(res.final_loss) and res.final_loss <= res.initial_loss and len(res.history) == 1
    assert set(OBJECTIVE_KEYS['views']) <= set(res.terms)
    assert all(math.isfinite(res.terms[k]) for k in OBJECTIVE_KEYS['views'][:5])
    assert res.seconds['views'] > 0 and set(res.seconds) >= {'run', 'pairs', 'tracks', 'host'}
