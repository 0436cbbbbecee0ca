"""GPU: crowd-dynamics statistics (piml_crowd_stats, piml_amd.crowdstats) against the float64 numpy restatement
(crowdstats_ref.py) on random slices, the recorded GC clips and simulated ensembles; determinism (two calls, graph replay,
member against a one-member call) and `simulate --stats`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crowdstats_ref as REF
from conftest import GOLDEN, REPO
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35'
GC_BOX = (5.0, 25.0, 15.0, 35.0)
SERIES = ('n', 'n_speed', 'sum_speed', 'sum_density')
FD = ('fd_count', 'fd_sum', 'fd_sum2')


def random_slices(S, T, N, seed, density=1.5):
    """positions uniform over a square holding ~density agents per m^2 (so the bins fill), absent agents (mask 0), present
    ones with a NaN or infinite position, non-finite velocities and masks that are neither 0 nor 1"""
    rng = np.random.default_rng(seed)
    side = np.sqrt(max(N, 1) / density)
    P = (rng.random((S, T, N, 2)) * side - 0.2 * side).astype(np.float32)
    V = rng.normal(0.0, 1.0, (S, T, N, 2)).astype(np.float32)
    M = (rng.random((S, T, N)) < 0.85).astype(np.float32)
    r = rng.random((S, T, N))
    P[(r < 0.03)] = np.nan
    P[(r >= 0.03) & (r < 0.04), 0] = np.inf
    M[(r >= 0.04) & (r < 0.05)] = 0.5
    P[(M == 0) & (rng.random((S, T, N)) < 0.5)] = np.nan
    q = rng.random((S, T, N))
    V[q < 0.05, 0] = np.nan
    V[(q >= 0.05) & (q < 0.08), 1] = -np.inf
    return P, V, M, side


def check_against_ref(st, P, V, M, n_active=None, **kw):
    """rho within 1e-5 of float64; series, diagram and map exact given the device's rho (float64 sums to 1e-12)"""
    want = REF.crowd_stats(P, V, M, n_active=n_active, **kw)
    got_rho, want_rho = st.density, want['density']
    assert np.array_equal(np.isnan(got_rho), np.isnan(want_rho))
    ok = ~np.isnan(want_rho)
    if ok.any():
        rel = np.abs(got_rho[ok].astype(np.float64) - want_rho[ok]) / np.abs(want_rho[ok].astype(np.float64))
        assert rel.max() <= 1e-5, rel.max()
    exact = REF.crowd_stats(P, V, M, n_active=n_active, rho=got_rho, **kw)
    for k in ('n', 'n_speed', 'fd_count'):
        assert np.array_equal(getattr(st, k), exact[k]), k
    for k in ('sum_speed', 'sum_density', 'fd_sum', 'fd_sum2'):
        np.testing.assert_allclose(getattr(st, k), exact[k], rtol=1e-12, atol=1e-300, err_msg=k)
    if kw.get('box') is None:
        assert st.map is None
    else:
        assert np.array_equal(st.map, exact['map'])
    return exact


# (1024 and 1025: a frame that just fills the staged tile and one that needs a second)
CASES = [(1, 8, 50), (63, 8, 50), (64, 4, 30), (65, 8, 50), (1000, 2, 6), (4097, 1, 3), (1024, 2, 3), (1025, 2, 3)]


@pytest.mark.parametrize('N,S,T', CASES)
def test_random_slices_against_numpy(N, S, T):
    from piml_amd.crowdstats import crowd_stats
    P, V, M, side = random_slices(S, T, N, seed=N)
    n_active = [N - (s * N) // (2 * S) for s in range(S)]           # member s sweeps its first n_active[s] slots
    box = (0.0, 0.55 * side, 0.1 * side, 0.7 * side)
    for kw in (dict(), dict(box=box, cell=0.37, frames=(1, T) if T > 1 else None, rho_bin=0.2, rho_bins=9)):
        st = crowd_stats(torch.tensor(P, device=DEV), torch.tensor(V, device=DEV), torch.tensor(M, device=DEV),
                         return_density=True, n_active=n_active, **kw)
        ex = check_against_ref(st, P, V, M, n_active=n_active, **kw)
        assert ex['n'].sum() > 0 or N == 1
    if N >= 1000:                        # the agents spread over several bins, the open-ended last one included
        assert (st.fd_count[:, -1] > 0).all() and ((st.fd_count > 0).sum(1) >= 3).all()


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.crowdstats import crowd_stats
    S, T, N = 5, 40, 300
    P, V, M, side = random_slices(S, T, N, seed=7)
    Pt, Vt, Mt = (torch.tensor(x, device=DEV) for x in (P, V, M))
    kw = dict(box=(0.0, side * 0.6, 0.0, side * 0.6), cell=0.5, return_density=True)
    a, b = crowd_stats(Pt, Vt, Mt, **kw), crowd_stats(Pt, Vt, Mt, **kw)
    names = SERIES + FD + ('map',)
    for k in names:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.density.view(np.uint32), b.density.view(np.uint32))
    # member m of the S-member call == an S = 1 call on member m (also through the (T, N, .) promotion)
    for m in range(S):
        one = crowd_stats(Pt[m], Vt[m], Mt[m], **kw)
        for k in names:
            assert np.array_equal(getattr(a, k)[m:m + 1], getattr(one, k)), (m, k)
        assert np.array_equal(a.density[m:m + 1].view(np.uint32), one.density.view(np.uint32))
    # graph replay == eager
    grid = (a.map.shape[2], a.map.shape[1])
    args = (Pt, Vt, Mt, 0.7, kw['box'], grid, 0.5, 0.25, 24, (0, T), True, None)
    eager = ops_metrics.crowd_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.crowd_stats_frames(*args)                    # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.crowd_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        x, y = v, cap[k]
        if v.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        elif v.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k
    assert np.array_equal(eager['n'].cpu().numpy(), a.n)


def test_library_rejects_bad_arguments():
    from piml_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 2, 3, 2, device=DEV)
    m = torch.ones(1, 2, 3, device=DEV)
    o64 = torch.zeros(64, device=DEV, dtype=torch.float64)
    ws = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()

    def call(S=1, T=2, N=3, t0=0, t1=2, R=0.7, box=0, x0=0., x1=1., y0=0., y1=1., h=0.5, gx=2, gy=2, rb=0.25, B=4,
             mp=True, wsb=4096):
        return L.piml_crowd_stats(p(x), p(x), p(m), None, S, T, N, t0, t1, R, box, x0, x1, y0, y1, h, gx, gy, rb, B,
                                  p(o64), p(o64), p(o64), p(o64), p(o64), p(o64), p(o64), p(o64) if mp else None, None,
                                  p(ws), wsb, torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(S=0), dict(T=0), dict(N=-1), dict(R=0.0), dict(R=-1.0), dict(R=float('nan')), dict(B=0),
                dict(B=257), dict(rb=0.0), dict(t0=1, t1=1), dict(t1=3), dict(t0=-1), dict(box=1, x1=0.),
                dict(box=1, y0=2.), dict(box=1, h=0.), dict(box=1, gx=0), dict(box=1, mp=False), dict(wsb=8)):
        assert call(**bad) == 1, bad
    assert L.piml_crowd_stats_workspace_bytes(-1, 2, 3) == -1


def _raw(name):
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return raw


def test_recorded_clips():
    from piml_amd.crowdstats import compare_crowd_stats, crowd_stats_of_raw
    out = []
    for name in (GC_CLIP, GC_CLIP + '_simulation'):
        raw = _raw(name)
        P, V, M = (x.numpy() for x in (raw.position, raw.velocity, raw.mask_p))
        for kw in (dict(), dict(box=GC_BOX, cell=0.5)):
            st = crowd_stats_of_raw(raw, return_density=True, **kw)
            check_against_ref(st, P, V, M, **kw)
            assert st.n.shape == (1, raw.num_steps) and st.n.max() >= 1
        out.append(st)
    c1 = compare_crowd_stats(out[0], out[1], min_count=20)
    c2 = compare_crowd_stats(out[0], out[1], min_count=20)
    assert c1 == c2
    assert c1['fd_bins'] >= 1 and all(np.isfinite(c1[k]) for k in ('fd_distance', 'map_distance', 'mean_speed_diff',
                                                                   'mean_density_diff'))


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


def _equal(a, b, names=SERIES + FD + ('map', 'slices')):
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names)


def test_simulated_ensembles(sim):
    from piml_amd.crowdstats import crowd_stats_of_raw
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to(DEV)
    kw = dict(box=GC_BOX, cell=0.5)
    ens = sim.simulate_ensemble(sc, 100, [0, 1, 2, 3])
    st = ens.crowd_stats(**kw)
    assert st.n.shape == (4, 100) and st.n.sum() > 0
    for m in range(4):
        mem = ens.member(m)
        one = mem.crowd_stats(**kw)
        assert _equal(st.member(m), one), m
        raw = crowd_stats_of_raw(mem.to_raw_data(), **kw)
        assert _equal(one, raw), m
    pool = st.pooled()
    assert pool.fd_count[0].sum() == st.fd_count.sum() and pool.slices[0] == 400
    # the same call on an MLAPM-driven ensemble, against the restatement
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    me = law.simulate_ensemble(sc, 60, [4, 5])
    ms = me.crowd_stats(return_density=True, **kw)
    cap = me.position.shape[2]
    check_against_ref(ms, me.position.cpu().numpy(), me.velocity.cpu().numpy(), me.mask_p.cpu().numpy(),
                      n_active=[min(n, cap) for n in me.spawned], **kw)


def test_simulate_cli_stats(tmp_path):
    from piml_amd.crowdstats import CrowdStats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'stats.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:2', '--frames', '40', '--out', clip,
                        '--stats', out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = CrowdStats.from_json(out)
    assert st.n.shape == (2, 40) and st.n.sum() > 0 and st.fd_count.sum() == st.n_speed.sum()
    assert not os.path.exists(clip.replace('{seed}', '0'))               # --stats writes no clip
    with open(out) as fh:
        assert json.load(fh)['pooled']['mean_speed'] > 0
