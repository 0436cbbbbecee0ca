"""GPU: time-to-collision and pair-distance statistics (piml_pair_stats, piml_amd.pairstats) against the numpy restatement
(pairstats_ref.py) on random slices, analytic placements and the recorded GC and UCY clips; determinism (two calls, graph
replay, member against a one-member call), ensembles against their members, and the two command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pairstats_ref as REF
from conftest import GOLDEN, REPO
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35'
UCY_CLIP = 'UCY_Dataset_time162-216_timeunit0.08'
GC_BOX = (5.0, 25.0, 15.0, 35.0)


def random_slices(S, T, N, seed, density=0.8):
    """positions uniform over a square of ~density agents per m^2, velocities ~ N(0, 1); absent agents, NaN and infinite
    positions, non-finite velocities and masks of 0.5"""
    rng = np.random.default_rng(seed)
    side = np.sqrt(max(N, 1) / density)
    P = (rng.random((S, T, N, 2)) * side).astype(np.float32)
    V = rng.normal(0.0, 1.0, (S, T, N, 2)).astype(np.float32)
    M = (rng.random((S, T, N)) < 0.85).astype(np.float32)
    r = rng.random((S, T, N))
    P[r < 0.03] = np.nan
    P[(r >= 0.03) & (r < 0.04), 0] = np.inf
    M[(r >= 0.04) & (r < 0.05)] = 0.5
    q = rng.random((S, T, N))
    V[q < 0.04, 0] = np.nan
    V[(q >= 0.04) & (q < 0.06), 1] = -np.inf
    return P, V, M, side


def _gpu(*xs):
    return [torch.tensor(np.asarray(x), device=DEV) for x in xs]


def check_against_ref(st, P, V, M, label, **kw):
    want = REF.pair_stats(P, V, M, **kw)
    frac = want['n_ambiguous'] / max(want['n_pairs'], 1)
    print(f'\n[pairstats] {label}: {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous ({frac:.2e})')
    assert frac <= 1e-3, frac
    REF.check(st, want, label)
    return want


# (1024 and 1025: a frame that just fills the staged tile and one that needs a second)
CASES = [(1500, 1, 4, (1, 2, 8)), (300, 3, 10, (2, 5)), (65, 2, 6, (1,)), (1, 1, 3, ()), (1024, 2, 3, (1,)), (1025, 2, 3, (1,))]


@pytest.mark.parametrize('N,S,T,lags', CASES)
def test_random_slices_against_numpy(N, S, T, lags):
    from piml_amd.pairstats import pair_stats
    P, V, M, side = random_slices(S, T, N, seed=N)
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    box = (0.1 * side, 0.6 * side, 0.2 * side, 0.9 * side)
    Pt, Vt, Mt = _gpu(P, V, M)
    for kw in (dict(lags=lags), dict(lags=lags, box=box, r_max=2.5, frames=(1, T), tau_bins=30, r_bins=40),
               dict(lags=lags, n_active=n_active, radius=0.3, tau_bin=0.2, tau_bins=25, r_bin=0.25, r_bins=20)):
        st = pair_stats(Pt, Vt, Mt, **kw)
        want = check_against_ref(st, P, V, M, f'N={N} S={S} T={T} {sorted(kw)}', **kw)
        assert st.nn.sum() == st.focal[:, 0].sum() and st.min_ttc.sum() == st.focal[:, 0].sum()
        if N >= 300:
            assert want['pairs'][:, 0].min() > 0 and want['ttc'][:, 0].sum() > 0 and want['overlap'][:, 0].sum() > 0
    if 8 in lags:                              # a lag past the window: no slices, zero counts
        assert (st.focal[:, 3] == 0).all() and (st.pairs[:, 3] == 0).all() and (st.ttc[:, 3] == 0).all()


def test_analytic_placements_are_exact():
    """head-on pairs at tau = (b + 0.3) 0.1 s, distance 0.56 + 0.2 b m (inside their bins), 10 m apart from each other;
    overlapping and receding pairs; r_max keeps each agent to its partner.  Every count exact against a hand count, the
    float32 and the float64 restatement"""
    from piml_amd.pairstats import pair_stats
    P, V, want_ttc, want_dist = [], [], np.zeros(100, np.int64), np.zeros(100, np.int64)
    for b in range(23):
        tau = (b + 0.3) * 0.1
        D = 0.5 + 2 * tau
        y = 10.0 * len(P) / 2
        P += [[0.0, y], [D, y]]
        V += [[1.0, 0.0], [-1.0, 0.0]]
        want_ttc[b] += 2
        want_dist[int(D / 0.05)] += 2
    y = 10.0 * len(P) / 2
    P += [[0.0, y], [0.33, y], [0.0, y + 10], [1.23, y + 10]]          # overlapping; receding
    V += [[1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]]
    want_dist[6] += 2
    want_dist[24] += 2
    P, V = np.array(P, np.float32)[None], np.array(V, np.float32)[None]
    M = np.ones(P.shape[:2], np.float32)
    st = pair_stats(*_gpu(P, V, M), lags=(), r_max=8.0)          # pairs of different groups (>= 10 m) skipped
    n = P.shape[1]
    assert st.focal.tolist() == [[n]] and st.pairs.tolist() == [[n]] and st.overlap.tolist() == [[2]]
    assert np.array_equal(st.ttc[0, 0], want_ttc) and np.array_equal(st.dist[0, 0], want_dist)
    assert np.array_equal(st.nn[0, :100], want_dist) and st.nn[0, 100] == 0
    assert np.array_equal(st.min_ttc[0, :100], want_ttc) and st.min_ttc[0, 100] == 4
    ref = REF.pair_stats(P, V, M, lags=(), r_max=8.0)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(st, k), ref[k]) and np.array_equal(getattr(st, k), ref['f32'][k]), k


def _raw(name):
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return raw


def test_recorded_clips():
    from piml_amd.pairstats import compare_pair_stats, pair_stats_of_raw
    out = {}
    for name, box in ((GC_CLIP, GC_BOX), (UCY_CLIP, None)):
        raw = _raw(name)
        P, V, M = (x.numpy() for x in (raw.position, raw.velocity, raw.mask_p))
        st = pair_stats_of_raw(raw, box=box)
        check_against_ref(st, P, V, M, name, box=box)
        assert st.focal[0, 0] > 0 and st.ttc[0, 0].sum() > 0 and st.ttc[0, 1:].sum() > 0
        out[name] = st
        p, n = st.energy_exponent()
        print(f'[pairstats] {name}: energy exponent {p:.3f} over {n} bins, overlap rate {st.overlap_rate():.4g}')
    c = compare_pair_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
    assert c == compare_pair_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
    assert np.isfinite(c['ttc_l1']) and np.isfinite(c['nn_l1'])


def _bits_equal(a, b, names=REF.OUTPUTS):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in names)


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.pairstats import pair_stats
    S, T, N = 4, 30, 400
    P, V, M, side = random_slices(S, T, N, seed=11)
    Pt, Vt, Mt = _gpu(P, V, M)
    kw = dict(lags=(3, 7, 20), box=(0.0, side * 0.7, 0.0, side * 0.7))
    a, b = pair_stats(Pt, Vt, Mt, **kw), pair_stats(Pt, Vt, Mt, **kw)
    assert _bits_equal(a, b)
    for m in range(S):
        assert _bits_equal(a.member(m), pair_stats(Pt[m], Vt[m], Mt[m], **kw)), m
    args = (Pt, Vt, Mt, 0.5, (3, 7, 20), 0.1, 100, 0.05, 100, None, kw['box'], (0, T), None)
    eager = ops_metrics.pair_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.pair_stats_frames(*args)                    # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.pair_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


def test_simulated_ensembles(sim):
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.pairstats import pair_stats_of_raw
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to(DEV)
    kw = dict(lags=(8, 24), box=GC_BOX)
    ens = sim.simulate_ensemble(sc, 100, [0, 1, 2])
    st = ens.pair_stats(**kw)
    assert st.focal.shape == (3, 3) and st.pairs[:, 0].sum() > 0
    for m in range(3):
        mem = ens.member(m)
        one = mem.pair_stats(**kw)
        assert _bits_equal(st.member(m), one), m
        assert _bits_equal(one, pair_stats_of_raw(mem.to_raw_data(), **kw)), m
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    me = law.simulate_ensemble(sc, 80, [4, 5])
    kw = dict(kw, r_bin=0.1, r_bins=50)                 # wider distance bins: fewer pairs near an edge
    ms = me.pair_stats(**kw)
    for m in range(2):
        assert _bits_equal(ms.member(m), me.member(m).pair_stats(**kw)), m
    cap = me.position.shape[2]
    check_against_ref(ms, me.position.cpu().numpy(), me.velocity.cpu().numpy(), me.mask_p.cpu().numpy(), 'MLAPM ensemble',
                      n_active=[min(n, cap) for n in me.spawned], **kw)


def test_simulate_cli_pair_stats(tmp_path):
    from piml_amd.pairstats import PairStats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'pairs.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:2', '--frames', '40', '--out', clip,
                        '--pair-stats', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = PairStats.from_json(out)
    assert st.focal.shape == (2, 4) and st.focal[:, 0].sum() > 0 and (st.focal[:, 1:] == 0).all()   # lags past 40 frames
    assert not os.path.exists(clip.replace('{seed}', '0'))
    assert '[pairstats] simulate --pair-stats' in p.stdout


def test_pairstats_cli(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'cli.json')
    data = os.path.join(GOLDEN, 'data', GC_CLIP + '_simulation.npy')
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.pairstats', '--data', data, '--ref', ref, '--box', 'auto',
                        '--lags', '16,32', '--out', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(out) as fh:
        d = json.load(fh)
    from piml_amd.pairstats import PairStats
    st = PairStats.from_json(d['data'])
    assert st.options['lags'] == (16, 32) and st.focal[0, 0] > 0
    assert set(d['compare']) >= {'ttc_l1', 'nn_l1', 'g_tau_max_diff', 'energy_exponent_diff', 'overlap_rate_diff'}
    assert 'energy exponent' in p.stdout
