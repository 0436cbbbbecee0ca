"""GPU: collective-motion statistics (piml_flow_stats, piml_amd.flowstats) against the numpy restatement (flowstats_ref.py)
on random slices, analytic placements and the recorded GC and UCY clips; determinism (two calls, graph replay, member
against a one-member call), ensembles against their members, and the two command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flowstats_ref as REF
from conftest import GOLDEN, REPO
from test_pairstats_gpu import GC_BOX, GC_CLIP, UCY_CLIP, _gpu, _raw, random_slices, sim  # noqa: F401  (sim: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COS30, SIN30 = float(np.float32(np.cos(np.pi / 6))), float(np.float32(np.sin(np.pi / 6)))
CAP = 1e-3                                    # the ambiguous share of pairs, as test_pairstats_gpu.py


def flow_slices(S, T, N, seed):
    """test_pairstats_gpu.random_slices, with a share of velocities below v_min (speeds of 0 .. 0.2 m/s on one agent in
    ten) and some with a component >= 1024"""
    P, V, M, side = random_slices(S, T, N, seed)
    rng = np.random.default_rng(seed + 1000)
    q = rng.random((S, T, N))
    slow = q < 0.10
    with np.errstate(invalid='ignore'):       # the non-finite velocities stay non-finite
        V[slow] = (V[slow] * (0.2 * rng.random((int(slow.sum()), 1))
                              / np.maximum(np.linalg.norm(V[slow], axis=-1, keepdims=True), 1e-6))).astype(np.float32)
    V[(q >= 0.10) & (q < 0.11), 0] = 1024.0
    V[(q >= 0.11) & (q < 0.12), 1] = -3000.0
    return P, V, M, side


def option_sets(S, T, N, side):
    """the three option sets of a random case: defaults; box + window + smaller r_max + fewer bins + oblique axis; n_active
    per member + another band, v_min and cell"""
    box = (0.1 * side, 0.6 * side, 0.2 * side, 0.9 * side)
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    return (dict(),
            dict(box=box, frames=(1, T), r_max=2.5, r_bins=40, axis=(COS30, SIN30)),
            dict(n_active=n_active, lane_width=0.8, lane_length=3.0, v_min=0.3, cell=0.7, box=box, axis=(0.0, 1.0)))


def check_against_ref(st, P, V, M, label, **kw):
    want = REF.flow_stats(P, V, M, **kw)
    frac = want['n_ambiguous'] / max(want['n_pairs'], 1)
    print(f'\n[flowstats] {label}: {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous ({frac:.2e}); float32 run '
          f'against float64 over the unambiguous: {want["f32_deviation"]}')
    assert frac <= CAP, frac
    REF.check(st, want, label)
    return want


# (1024 and 1025: a frame that just fills the staged tile and one that needs a second)
CASES = [(1500, 1, 4), (300, 3, 10), (65, 2, 6), (1, 1, 3), (1024, 2, 3), (1025, 2, 3)]


@pytest.mark.parametrize('N,S,T', CASES)
def test_random_slices_against_numpy(N, S, T):
    from piml_amd.flowstats import flow_stats
    P, V, M, side = flow_slices(S, T, N, seed=N)
    Pt, Vt, Mt = _gpu(P, V, M)
    for kw in option_sets(S, T, N, side):
        st = flow_stats(Pt, Vt, Mt, **kw)
        check_against_ref(st, P, V, M, f'N={N} S={S} T={T} {sorted(kw)}', **kw)
        if N >= 300:
            assert st.corr_pairs.sum() > 0 and st.lane_n.sum() > 0 and st.lane_opp.sum() > 0
            assert st.map_n is None or st.map_n.sum() > 0
    assert st.map_n is not None
    if N == 1:
        assert st.corr_pairs.sum() == 0 and st.lane_n.sum() == 0


def test_analytic_placements_are_exact():
    """two opposite lanes of 8 along x, 1.23 m between neighbours, 2.24 m apart (beyond lane_width 0.5): phi = 1 for every
    agent, C = +1 within a lane and -1 across; then one file of 6 with strictly alternating directions at 0.73 m.  Positions
    sit well inside bins and bands; every output is the hand count."""
    from piml_amd.flowstats import Q, flow_stats
    n, gap = 8, 1.23
    P = [[1.05 + gap * k, 2.2] for k in range(n)] + [[1.05 + gap * k, 4.44] for k in range(n)]
    V = [[1.3, 0.0]] * n + [[-0.9, 0.0]] * n
    P, V = np.array(P, np.float32)[None], np.array(V, np.float32)[None]
    M = np.ones(P.shape[:2], np.float32)
    box = (0.0, 12.0, 0.0, 6.0)
    st = flow_stats(*_gpu(P, V, M), box=box)
    want_pairs, want_sum = np.zeros(60, np.int64), np.zeros(60, np.int64)
    band = 0
    for i in range(2 * n):
        for j in range(2 * n):
            if i == j:
                continue
            r = float(np.hypot(*(P[0, j].astype(np.float64) - P[0, i])))
            same_lane = (i < n) == (j < n)
            if r < 6.0:
                want_pairs[int(r / 0.1)] += 1
                want_sum[int(r / 0.1)] += Q if same_lane else -Q
            if same_lane and abs(P[0, j, 0] - P[0, i, 0]) < 5.0:
                band += 1
    assert np.array_equal(st.corr_pairs[0], want_pairs) and np.array_equal(st.corr_sum[0], want_sum)
    assert st.lane_n.tolist() == [[2 * n]] and st.lane_sum.tolist() == [[2 * n * Q]]
    assert st.lane_same.tolist() == [[band]] and st.lane_opp.tolist() == [[0]]
    assert st.dir_plus.tolist() == [[n]] and st.dir_minus.tolist() == [[n]]
    assert st.map_n.sum() == 2 * n and st.map_n[0, 4].sum() == n and st.map_n[0, 8].sum() == n
    assert st.map_vx[0, 4].sum() == n * int(round(float(np.float32(1.3)) * Q)) and st.map_vy.sum() == 0
    assert st.map_vx[0, 8].sum() == -n * int(round(float(np.float32(0.9)) * Q))
    c = st.velocity_correlation(min_count=1)
    assert set(c[np.isfinite(c)].tolist()) == {1.0, -1.0}
    ref = REF.flow_stats(P, V, M, box=box)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(st, k), ref[k]) and np.array_equal(getattr(st, k), ref['f32'][k]), k
    # strictly alternating directions in one file along y (axis 'y'), 0.73 m apart, lane_length 1.5: neighbours at 0.73 and 1.46
    m = 6
    P = np.array([[3.0, 1.0 + 0.73 * k] for k in range(m)], np.float32)[None]
    V = np.array([[0.0, 1.0 if k % 2 == 0 else -1.0] for k in range(m)], np.float32)[None]
    st = flow_stats(*_gpu(P, V, np.ones((1, m), np.float32)), axis='y', lane_length=1.5)
    ns = [sum(1 for j in range(m) if j != i and abs(j - i) == 2) for i in range(m)]
    no = [sum(1 for j in range(m) if j != i and abs(j - i) == 1) for i in range(m)]
    phi = sum(int(np.rint(np.float32(np.float32((a - b) / np.float32(a + b)) ** 2) * np.float32(Q))) for a, b in zip(ns, no))
    assert st.lane_same.tolist() == [[sum(ns)]] and st.lane_opp.tolist() == [[sum(no)]] and st.lane_n.tolist() == [[m]]
    assert st.lane_sum.tolist() == [[phi]] and st.dir_plus.tolist() == [[3]] and st.dir_minus.tolist() == [[3]]
    assert st.map_n is None and st.corr_pairs.sum() == m * (m - 1)
    assert st.corr_sum.sum() == Q * sum(1 if (i - j) % 2 == 0 else -1 for i in range(m) for j in range(m) if i != j)


def test_recorded_clips():
    from piml_amd.flowstats import compare_flow_stats, flow_stats_of_raw
    out = {}
    for name, box in ((GC_CLIP, GC_BOX), (UCY_CLIP, None)):
        raw = _raw(name)
        P, V, M = (x.numpy() for x in (raw.position, raw.velocity, raw.mask_p))
        st = flow_stats_of_raw(raw, box=box)
        check_against_ref(st, P, V, M, name, box=box)
        assert st.corr_pairs.sum() > 0 and st.lane_n.sum() > 0
        out[name] = st
        print(f'[flowstats] {name}: correlation length {st.correlation_length():.3f} m, lane order {st.lane_order()[1]:.4f}, '
              f'same-direction fraction {st.same_direction_fraction():.4f} (chance {st.chance_same_fraction():.4f})')
    c = compare_flow_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
    assert c == compare_flow_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
    assert np.isfinite(c['corr_max_diff']) and np.isfinite(c['lane_order_diff']) and c['flow_distance'] is None


def _bits_equal(a, b, names=REF.OUTPUTS):
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names)


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.flowstats import flow_stats
    S, T, N = 3, 30, 400
    P, V, M, side = flow_slices(S, T, N, seed=11)
    Pt, Vt, Mt = _gpu(P, V, M)
    box = (0.0, side * 0.7, 0.0, side * 0.7)
    kw = dict(box=box, axis=(COS30, SIN30))
    a, b = flow_stats(Pt, Vt, Mt, **kw), flow_stats(Pt, Vt, Mt, **kw)
    assert _bits_equal(a, b) and a.corr_pairs.sum() > 0 and a.map_n.sum() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), flow_stats(Pt[m], Vt[m], Mt[m], **kw)), m
    args = (Pt, Vt, Mt, 0.1, 0.1, 60, 6.0, (COS30, SIN30), 0.5, 5.0, box, REF.grid_shape(box, 0.5), 0.5, (0, T), None)
    eager = ops_metrics.flow_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.flow_stats_frames(*args)                    # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.flow_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


def test_simulated_ensembles(sim):
    """flow statistics use the stored velocities of a run; a clip written by to_raw_data keeps them, so every
    output is compared"""
    from piml_amd.flowstats import flow_stats_of_raw
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to(DEV)
    kw = dict(box=GC_BOX, axis='auto')
    ens = sim.simulate_ensemble(sc, 100, [0, 1, 2])
    st = ens.flow_stats(**kw)
    assert st.lane_n.shape == (3, 100) and st.corr_pairs.sum() > 0
    fixed = dict(kw, axis=st.options['axis'])           # 'auto' is taken over all members: hand a member the same axis
    for m in range(3):
        mem = ens.member(m)
        one = mem.flow_stats(**fixed)
        assert _bits_equal(st.member(m), one), m
        assert _bits_equal(one, flow_stats_of_raw(mem.to_raw_data(), **fixed)), m
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    cw = SCENARIOS['crosswalk']().to(DEV)
    me = law.simulate_ensemble(cw, 80, [4, 5, 6])
    ms = me.flow_stats()
    for m in range(3):
        assert _bits_equal(ms.member(m), me.member(m).flow_stats()), m
    cap = me.position.shape[2]
    check_against_ref(ms, me.position.cpu().numpy(), me.velocity.cpu().numpy(), me.mask_p.cpu().numpy(),
                      'MLAPM crosswalk ensemble', n_active=[min(n, cap) for n in me.spawned])
    print(f'[flowstats] MLAPM crosswalk, 3 x 80 frames: lane order {ms.lane_order()[1]:.4f}, same-direction fraction '
          f'{ms.same_direction_fraction():.4f} (chance {ms.chance_same_fraction():.4f})')


def test_simulate_cli_flow_stats(tmp_path):
    from piml_amd.flowstats import FlowStats, compare_flow_stats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'flow.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:2', '--frames', '40', '--out', clip,
                        '--flow-stats', out, '--flow-axis', 'auto'], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = FlowStats.from_json(out)
    assert st.lane_n.shape == (2, 40) and st.corr_pairs.shape == (2, 60) and st.dir_plus.sum() + st.dir_minus.sum() > 0
    assert not os.path.exists(clip.replace('{seed}', '0'))
    assert '[flowstats] simulate --flow-stats' in p.stdout
    c = compare_flow_stats(st, st)
    assert all(v == 0 for k, v in c.items() if k not in ('corr_bins', 'flow_distance') and np.isfinite(v))


def test_flowstats_cli(tmp_path):
    from piml_amd.flowstats import FlowStats, compare_flow_stats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'cli.json')
    data = os.path.join(GOLDEN, 'data', GC_CLIP + '_simulation.npy')
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.flowstats', '--data', data, '--ref', ref, '--box', 'auto',
                        '--axis', 'auto', '--out', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(out) as fh:
        d = json.load(fh)
    st, rs = FlowStats.from_json(d['data']), FlowStats.from_json(d['ref'])
    assert st.options['axis'] == rs.options['axis'] and st.corr_pairs.sum() > 0 and st.map_n.sum() > 0
    assert set(d['compare']) >= {'corr_max_diff', 'correlation_length_diff', 'lane_order_diff',
                                 'excess_same_fraction_diff', 'flow_distance'}
    c = compare_flow_stats(st, st)
    assert c['corr_max_diff'] == 0 and c['lane_order_diff'] == 0 and c['excess_same_fraction_diff'] == 0 \
        and c['flow_distance'] == 0
    assert 'lane order' in p.stdout
