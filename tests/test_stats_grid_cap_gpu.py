"""GPU: a second trip round the grid-capped loops that keep workgroup state in LDS from one item to the next --
track_stats_kernel over tracks (h_acc, span, red) and crowd_density_body over slices (the per-wave diagram rows, red_*).
Both cap their grid at *_MAX_GRID workgroups (read from the sources by stats_runs_shapes.py); a call with more items than
that gives the first workgroups a second item, which no other test does.  The oracle is the same call split by members so
that no part reaches the cap, compared bit for bit: the integer outputs do not depend on the order of their atomic adds,
and each slice's float64 sums are formed in a fixed order inside its own workgroup."""
import time

import numpy as np
import pytest
import torch

import stats_runs_shapes as SH
import trackstats_ref
from test_crowdstats_gpu import FD, SERIES, random_slices as crowd_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _tracks(S, T, N, seed):
    """random walks whose step noise grows with the member (the last member's fills the acceleration bins up to the open one),
    with absent frames, a few non-finite positions and about one track in four absent throughout"""
    rng = np.random.default_rng(seed)
    sigma = (0.004 * (1 + np.arange(S) % 5)).astype(np.float32)
    sigma[-1] = 0.03
    steps = rng.normal(0.0, 1.0, (S, T, N, 2)).astype(np.float32) * sigma[:, None, None, None] + np.float32(0.05)
    P = (rng.random((S, 1, N, 2)) * 40.0).astype(np.float32) + np.cumsum(steps, 1, dtype=np.float32)
    M = (rng.random((S, T, N)) < 0.9).astype(np.float32)
    P[rng.random((S, T, N)) < 0.01] = np.nan
    empty = rng.random((S, N)) < 0.25
    M[np.broadcast_to(empty[:, None, :], M.shape)] = 0.0
    return P, M, empty


def test_track_stats_second_trip_equals_split_call():
    from piml_amd import ops_metrics
    t = SH.TRACKS
    S, T, N, NL = t['S'], t['T'], t['N'], t['n_lags']
    cap = SH.constant('TS_MAX_GRID')
    assert cap < S * N <= 2 * cap and cap % N == 0 and cap // N == S - 1       # the second tracks: all of the last member
    assert all((b - a) * N <= cap for a, b in t['halves']) and [h for h in t['halves']] == [(0, 9), (9, S)]
    P, M, empty = _tracks(S, T, N, seed=5)
    Pt, Mt = torch.tensor(P, device=DEV), torch.tensor(M, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one = ops_metrics.track_stats_frames(Pt, Mt, n_lags=NL)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    print(f'\n[stats grid cap] tracks: {S * N} tracks over {cap} workgroups, device call {sec * 1e3:.1f} ms')
    one = {k: v.cpu().numpy() for k, v in one.items()}
    assert set(one) == set(trackstats_ref.OUTPUTS)
    # the second trips are not vacuous: tracks absent throughout (frames == 0 -> continue) and acceleration items in many bins
    last = S - 1
    share = (one['trk_frames'][last] == 0).mean()
    assert 0.2 < share < 0.3 and (one['trk_frames'][last][empty[last]] == 0).all()
    assert (one['trk_first'][last][one['trk_frames'][last] == 0] == -1).all()
    assert (one['acc'][last] > 0).sum() >= 20 and one['acc'][last, -1] > 0 and one['acc_sum'][last] > 0
    assert (one['acc'][0] > 0).sum() >= 5 and one['ac_n'][last].min() > 0 and one['msd_n'][last].min() > 0
    assert one['trk_path'][last].max() > 0 and one['trk_net'][last].max() > 0 and one['trk_steps'][last].max() == T - 1
    assert len({one['acc'][s].tobytes() for s in range(S)}) == S
    parts = []
    for a, b in t['halves']:
        part = ops_metrics.track_stats_frames(Pt[a:b], Mt[a:b], n_lags=NL)
        parts.append({k: v.cpu().numpy() for k, v in part.items()})
    for k in trackstats_ref.OUTPUTS:
        assert np.array_equal(one[k], np.concatenate([p[k] for p in parts], 0)), k


def test_crowd_stats_second_trip_equals_member_calls():
    from piml_amd.crowdstats import crowd_stats
    c = SH.CROWD
    S, T, N, B = c['S'], c['T'], c['N'], c['rho_bins']
    cap = SH.constant('CD_MAX_GRID')
    assert cap < S * T <= 2 * cap and T <= cap and cap // T == S - 1           # the second slices: the last member's
    P, V, M, side = crowd_slices(S, T, N, seed=9)
    Pt, Vt, Mt = (torch.tensor(x, device=DEV) for x in (P, V, M))
    kw = dict(box=(-0.1 * side, 0.6 * side, -0.1 * side, 0.6 * side), cell=0.25, rho_bin=0.45, rho_bins=B, return_density=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one = crowd_stats(Pt, Vt, Mt, **kw)
    torch.cuda.synchronize()
    print(f'\n[stats grid cap] crowd: {S * T} slices over {cap} workgroups, call with its copies '
          f'{(time.perf_counter() - t0) * 1e3:.1f} ms')
    second = cap - (S - 1) * T                                   # frames of the last member from here on are second trips
    assert 0 < second < T - 1000
    assert one.n[-1, second:].sum() > 1000 and one.n_speed[-1, second:].sum() > 1000 and one.sum_speed[-1, second:].sum() > 0
    assert (one.fd_count > 0).sum(1).min() >= 2 and one.map.sum((1, 2)).min() > 0
    assert np.isfinite(one.density[-1, second:]).sum() > 1000
    assert len({one.fd_count[s].tobytes() for s in range(S)}) == S
    members = [crowd_stats(Pt[m:m + 1], Vt[m:m + 1], Mt[m:m + 1], **kw) for m in range(S)]
    for k in SERIES + FD + ('map',):
        x, y = getattr(one, k), np.concatenate([getattr(m, k) for m in members], 0)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), k
    assert np.array_equal(one.density.view(np.uint32), np.concatenate([m.density for m in members], 0).view(np.uint32))
