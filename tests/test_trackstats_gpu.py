"""GPU: track statistics (piml_track_stats, piml_amd.trackstats) against the numpy restatement (trackstats_ref.py) on
random tracks, analytic tracks and the recorded GC and UCY clips; determinism (two calls, graph replay, member against a
one-member call), ensembles and sweeps against their members, and the two command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import trackstats_ref as REF
from conftest import GOLDEN, REPO
from test_pairstats_gpu import GC_CLIP, UCY_CLIP, _gpu, _raw

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 1e-3                                    # the ambiguous share of items, as test_pairstats_gpu.py
Q = REF.Q


def _consts():
    from piml_amd import ops_metrics
    return ops_metrics.TRACK_TILE, ops_metrics.TRACK_LAG_LANES, ops_metrics.TRACK_MAX_LAGS


def option_sets(S, T, N, n_lags):
    """the three option sets of a random case: defaults with the case's lags; window + n_active per member + another v_min,
    other bins and d_max = 3 m; one lag"""
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    window = dict(frames=(1, T)) if T > 1 else {}
    return (dict(n_lags=n_lags),
            dict(n_lags=n_lags, n_active=n_active, v_min=0.3, acc_bin=0.4, acc_bins=12, d_max=3.0, **window),
            dict(n_lags=1))


def check_against_ref(st, P, M, label, **kw):
    want = REF.track_stats(P, M, **kw)
    frac = want['n_ambiguous'] / max(want['n_items'], 1)
    print(f'\n[trackstats] {label}: {want["n_items"]} items, {want["n_ambiguous"]} ambiguous ({frac:.2e}; lag / MSD pairs, '
          f'acceleration items, steps: {want["kinds"]}); float32 run against float64 over the unambiguous: '
          f'{want["f32_deviation"]}')
    assert frac <= CAP, frac
    dev = REF.check(st, want, label)
    # the device is expected to be the float32 run, bit for bit, ambiguous items or not: recorded, asserted by check() where
    # nothing is ambiguous
    print(f'[trackstats] {label}: device == float32 run bit for bit: {all(v[1] == 0 for v in dev.values())}')
    return want


# N, S, T, n_lags (None: set from the kernel's constants below), centred on the origin
CASES = [(1, 1, 3, 4, False), (1, 1, 1, 1, False), (65, 3, 300, 130, False), (300, 2, 40, 16, False), (1500, 1, 12, 32, False),
         (7, 2, 'tile', 64, False), (65, 3, 300, 'max', False), (65, 3, 300, 'pass+1', False), (65, 2, 300, 130, True),
         (300, 2, 40, 16, True)]


@pytest.mark.parametrize('N,S,T,n_lags,centred', CASES)
def test_random_tracks_against_numpy(N, S, T, n_lags, centred):
    from piml_amd.trackstats import track_stats
    tile, lanes, max_lags = _consts()
    n_lags = {'max': max_lags, 'pass+1': lanes + 1}.get(n_lags, n_lags)
    T = tile + 1 + n_lags if T == 'tile' else T
    P, M = REF.random_tracks(S, T, N, seed=N + T, centred=centred)
    if T > tile:
        P[:, :, 0], M[:, :, 0] = P[0, :, 0], 1.0          # slot 0 of every member is there throughout (member 0's walk)
        P[:, :, 0][~np.isfinite(P[:, :, 0]) | (np.abs(P[:, :, 0]) >= 65536)] = 700.0
    Pt, Mt = _gpu(P, M)
    for kw in option_sets(S, T, N, n_lags):
        st = track_stats(Pt, Mt, **kw)
        check_against_ref(st, P, M, f'N={N} S={S} T={T} centred={centred} {sorted(kw)} n_lags={kw["n_lags"]}', **kw)
        if N >= 65:
            assert st.ac_n.sum() > 0 and st.msd_n.sum() > 0 and st.acc.sum() > 0 and st.trk_path.sum() > 0
        if 'd_max' in kw and T >= 40:
            assert st.msd_far.sum() > 0
    if T > tile:
        full = track_stats(Pt, Mt, n_lags=n_lags)
        assert (full.trk_frames[:, 0] == T).all() and full.msd_n[0, n_lags - 1] >= T - n_lags     # pairs straddle the tile edge
    if T == 3:
        assert st.ac_n.sum() == 0                          # one lag, at most two steps... and the rows of lags past the window
        first = track_stats(Pt, Mt, n_lags=4)
        assert (first.ac_n[:, 2:] == 0).all() and (first.msd_n[:, 2:] == 0).all() and (first.msd_far[:, 2:] == 0).all()
    if T == 1:
        assert st.trk_steps.sum() == 0 and st.acc.sum() == 0 and st.msd_n.sum() == 0


def test_analytic_tracks_are_exact():
    """the hand-counted tracks of test_trackstats.py on the device: a straight track, an oblique one, an out-and-back one,
    one with a hole and a standing agent, in one call; hand counts == device == both restatements"""
    from piml_amd.trackstats import track_stats
    T, NL, step = 21, 12, 0.125
    there = set(range(0, 6)) | set(range(8, 15))
    cols = [[(10.0 + step * t, 3.0) for t in range(T)],
            [(10.0 + 0.09375 * t, 6.0 + 0.125 * t) for t in range(T)],
            [(10.0 + step * min(t, T - 1 - t), 2.0) for t in range(T)],
            [(10.0 + step * t, 1.0) if t in there else None for t in range(T)],
            [(7.0, 7.0)] * T]
    P, M = np.zeros((1, T, 5, 2), np.float32), np.zeros((1, T, 5), np.float32)
    for n, col in enumerate(cols):
        for t, p in enumerate(col):
            if p is not None:
                P[0, t, n], M[0, t, n] = p, 1.0
    st = track_stats(*_gpu(P, M), n_lags=NL, d_max=0.9)
    ref = REF.track_stats(P, M, n_lags=NL, d_max=0.9)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(st, k), ref[k]) and np.array_equal(getattr(st, k), ref['f32'][k]), k
    steps = [set(range(T - 1)), set(range(T - 1)), set(range(T - 1)), {t for t in there if t + 1 in there}]
    frames = [set(range(T))] * 3 + [there, set(range(T))]
    per_step = [16384, 25600, None, 16384, 0]              # |u|^2 Q of the constant-velocity tracks
    for L in range(1, NL + 1):
        ac_n = sum(sum(1 for t in s if t + L in s) for s in steps)
        turn = sum(1 if (t < 10) == (t + L < 10) else -1 for t in steps[2] if t + L in steps[2])
        ac_sum = sum(sum(1 for t in s if t + L in s) for s in (steps[0], steps[1], steps[3])) + turn
        assert st.ac_n[0, L - 1] == ac_n and st.ac_sum[0, L - 1] == ac_sum * Q, L
        near = far = total = 0
        for n, fr in enumerate(frames):
            for t in fr:
                if t + L not in fr:
                    continue
                d2q = per_step[n] * L * L if n != 2 else 16384 * (min(t + L, T - 1 - t - L) - min(t, T - 1 - t)) ** 2
                if d2q < 0.81 * Q:
                    near, total = near + 1, total + d2q
                else:
                    far += 1
        assert (st.msd_n[0, L - 1], st.msd_far[0, L - 1], st.msd_sum[0, L - 1]) == (near, far, total), L
    assert st.acc[0, 0] == 4 * (T - 2) - 1 + 9 and st.acc[0, 40] == 1 and st.acc.sum() == st.acc[0, 0] + 1
    assert st.trk_frames[0].tolist() == [T, T, T, 13, T] and st.trk_steps[0].tolist() == [T - 1, T - 1, T - 1, 11, T - 1]
    assert st.trk_first[0].tolist() == [0] * 5 and st.trk_last[0].tolist() == [T - 1, T - 1, T - 1, 14, T - 1]
    assert st.trk_path[0].tolist() == [20 * Q // 8, 20 * 163840, 20 * Q // 8, 11 * Q // 8, 0]
    assert st.trk_net[0].tolist() == [20 * Q // 8, 20 * 163840, 0, 14 * Q // 8, 0]
    assert st.straight_hist[0, 0].tolist() == [1] + [0] * 18 + [3] and st.straight_n[0].tolist() == [4, 0]
    assert st.heading_autocorrelation(min_count=1)[9] < 1.0 and st.mean_straightness() == pytest.approx(0.75)


def test_recorded_clips():
    from piml_amd.trackstats import compare_track_stats, track_stats_of_raw
    out = {}
    for name in (GC_CLIP, UCY_CLIP):
        raw = _raw(name)
        P, M = raw.position.numpy(), raw.mask_p.numpy()
        st = track_stats_of_raw(raw, n_lags=64)
        assert st.options['dt'] == float(raw.time_unit)
        check_against_ref(st, P, M, name, n_lags=64, dt=float(raw.time_unit))
        assert st.ac_n.sum() > 0 and st.msd_n.sum() > 0 and st.acc.sum() > 0
        out[name] = st
        print(f'[trackstats] {name}: persistence time {st.persistence_time():.3f} s, MSD exponent {st.msd_exponent():.3f}, '
              f'mean acceleration {st.mean_acceleration():.4f} m/s^2, mean straightness {st.mean_straightness():.4f}')
    if out[GC_CLIP].options['dt'] == out[UCY_CLIP].options['dt']:
        c = compare_track_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
        again = compare_track_stats(out[GC_CLIP], out[UCY_CLIP], min_count=20)
        assert json.dumps(c) == json.dumps(again) and np.isfinite(c['acc_l1'])          # (a NaN is not equal to itself)
    else:
        with pytest.raises(ValueError):
            compare_track_stats(out[GC_CLIP], out[UCY_CLIP])


def _bits_equal(a, b, names=None):
    from piml_amd.trackstats import ARRAYS
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names or ARRAYS)


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.trackstats import track_stats
    S, T, N = 3, 200, 150
    P, M = REF.random_tracks(S, T, N, seed=11)
    Pt, Mt = _gpu(P, M)
    kw = dict(n_lags=140, frames=(2, T - 1), d_max=4.0)
    a, b = track_stats(Pt, Mt, **kw), track_stats(Pt, Mt, **kw)
    assert _bits_equal(a, b) and a.ac_n.sum() > 0 and a.msd_far.sum() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), track_stats(Pt[m], Mt[m], **kw)), m
    args = (Pt, Mt, 0.08, 0.1, 140, 4.0, 0.25, 40, (2, T - 1), None)
    eager = ops_metrics.track_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.track_stats_frames(*args)                   # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.track_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


def test_simulated_ensembles_and_sweeps():
    """track statistics use positions only, so a clip written by to_raw_data gives the same statistics as the run"""
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.trackstats import ADDITIVE, TRACK_ROWS, track_stats_of_raw
    truth = dict(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    off = dict(truth, tau=1.0)
    cw = SCENARIOS['crosswalk']().to(DEV)
    kw = dict(n_lags=32)
    me = MLAPM(**truth).simulate_ensemble(cw, 80, [4, 5, 6])
    ms = me.track_stats(**kw)
    assert ms.members == 3 and ms.options['dt'] == float(me.time_unit) and ms.ac_n.sum() > 0 and ms.acc.sum() > 0
    for m in range(3):
        mem = me.member(m)
        one = mem.track_stats(**kw)
        assert _bits_equal(ms.member(m), one), m
        raw = track_stats_of_raw(mem.to_raw_data(), **kw)          # the clip holds the member's num_agents slots only
        n = mem.num_agents
        assert _bits_equal(one, raw, ADDITIVE), m
        for k in TRACK_ROWS:
            assert np.array_equal(getattr(one, k)[:, :n], getattr(raw, k)), (m, k)
            assert (getattr(one, k)[:, n:] == (-1 if k in ('trk_first', 'trk_last') else 0)).all(), (m, k)
    cap = me.position.shape[2]
    check_against_ref(ms, me.position.cpu().numpy(), me.mask_p.cpu().numpy(), 'MLAPM crosswalk ensemble',
                      n_active=[min(n, cap) for n in me.spawned], dt=float(me.time_unit), **kw)
    print(f'[trackstats] MLAPM crosswalk, 3 x 80 frames: persistence time {ms.persistence_time():.3f} s, MSD exponent '
          f'{ms.msd_exponent(tau_range=(0.3, 2.5)):.3f}, mean acceleration {ms.mean_acceleration():.4f} m/s^2')
    # a sweep's candidates against their single-law ensembles
    seeds = [0, 1, 2]
    sw = MLAPM.simulate_sweep(cw, 48, [truth, off], seeds)
    ss = sw.track_stats(**kw)
    assert ss.members == 6
    for c, law in enumerate((truth, off)):
        ens = MLAPM(**law).simulate_ensemble(cw, 48, seeds, capacity=sw.capacity)
        assert _bits_equal(ss.select(sw.members_of(c)).pooled(), ens.track_stats(**kw).pooled()), c
        assert _bits_equal(sw.candidate(c).track_stats(**kw), ss.select(sw.members_of(c))), c


def test_simulate_cli_track_stats(tmp_path):
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.trackstats import TrackStats
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'tracks.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scenario', 'crosswalk', '--seeds',
                        '0:2', '--frames', '40', '--out', clip, '--track-stats', out], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = TrackStats.from_json(out)
    assert st.members == 2 and st.ac_n.shape == (2, 128) and st.acc.shape == (2, 41) and st.msd_n.sum() > 0
    assert not os.path.exists(clip.replace('{seed}', '0'))
    assert '[trackstats] simulate --track-stats' in p.stdout
    from piml_amd.simulate import load_mlapm_params
    own = MLAPM(**load_mlapm_params(None)).simulate_ensemble(SCENARIOS['crosswalk']().to(DEV), 40, [0, 1]).track_stats()
    assert _bits_equal(st, own), 'the JSON of the command line differs from the in-process statistics'
    assert st.options == own.options


def test_trackstats_cli(tmp_path):
    from piml_amd.trackstats import ADDITIVE, TrackStats, compare_track_stats, track_stats_of_raw
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'cli.json')
    data = os.path.join(GOLDEN, 'data', GC_CLIP + '_simulation.npy')
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.trackstats', '--data', data, '--ref', ref, '--lags', '48', '--out',
                        out], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(out) as fh:
        d = json.load(fh)
    st, rs = TrackStats.from_json(d['data']), TrackStats.from_json(d['ref'])
    assert st.options['n_lags'] == 48 and st.trk_path is None and rs.trk_path is not None and st.msd_n.sum() > 0
    assert set(d['compare']) == {'heading_ac_max_diff', 'heading_ac_bins', 'persistence_time_diff', 'msd_exponent_diff',
                                 'acc_l1', 'mean_acceleration_diff', 'straightness_l1', 'speed_l1', 'duration_l1'}
    from piml_amd.crowdstats import _load
    assert _bits_equal(rs, track_stats_of_raw(_load(ref), n_lags=48))
    assert _bits_equal(st, track_stats_of_raw(_load(data), n_lags=48).pooled(), ADDITIVE)
    c = compare_track_stats(st, st)
    assert c['heading_ac_max_diff'] == 0 and c['acc_l1'] == 0 and c['straightness_l1'] == 0
    assert 'persistence time' in p.stdout and 'data vs ref' in p.stdout
