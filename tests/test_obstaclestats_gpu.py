"""GPU: obstacle statistics (piml_obstacle_stats, piml_amd.obstaclestats) against the numpy restatement (obstaclestats_ref.py)
on random slices, the analytic scene and the recorded GC and UCY clips; determinism (two calls, graph replay, member against
a one-member call, a permutation of the obstacle points), a short GC ensemble against its members and the two command lines,
and the check that motivated the family: the MLAPM law, which has no obstacle term, hits the GC walls at least as often as
the recorded pedestrians do."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import obstaclestats_ref as REF
from conftest import GOLDEN, REPO
from test_pairstats_gpu import GC_CLIP, UCY_CLIP, _gpu, _raw, random_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 1e-3                                    # the ambiguous share of items, as test_pairstats_gpu.py
Q = REF.Q
SEEDS, FRAMES = [0, 1, 2], 40                 # the short GC ensemble


def _tile():
    from piml_amd import ops_metrics
    return ops_metrics.OBS_TILE


def check_against_ref(st, P, V, M, obs, label, **kw):
    want = REF.obstacle_stats(P, V, M, obs, **kw)
    frac = want['n_ambiguous'] / max(want['n_items'], 1)
    print(f'\n[obstaclestats] {label}: {want["n_items"]} items, {want["n_ambiguous"]} ambiguous ({frac:.2e})')
    assert frac <= CAP, frac
    dev = REF.check(st, want, label)
    # the device is expected to be the float32 run, bit for bit, ambiguous items or not: recorded, asserted by check() for
    # every member without an ambiguous item
    print(f'[obstaclestats] {label}: device == float32 run bit for bit: {all(v[0] == 0 for v in dev.values())}')
    host = REF.host_rows({k: getattr(st, k) for k in REF.TRACK_ROWS}, st.options['r_bin'], st.options['r_bins'])
    for k in REF.HISTS:
        assert np.array_equal(getattr(st, k), host[k]), (label, k)
    return want


def option_sets(S, T, N, side):
    """the three option sets of a random case: defaults; window + n_active per member + box + other radii and bins; one bin"""
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    window = dict(frames=(1, T)) if T > 1 else {}
    return (dict(),
            dict(n_active=n_active, box=(0.1 * side, 0.9 * side, 0.05 * side, 0.8 * side), radius=0.4, hit_radius=0.2, r_bin=0.25,
                 r_bins=12, tau_bin=0.3, tau_bins=9, **window),
            dict(r_bins=1, tau_bins=1))


# N, S, T, O (None: one more than a tile), the share of NaN / infinite obstacle points
# (N = 1100: more slots than one focal compaction takes, so its second round runs)
CASES = [(1, 1, 1, 1, 0.0), (1, 1, 2, 1, 0.0), (65, 3, 40, 7, 0.0), (300, 2, 12, None, 0.0), (65, 2, 9, 900, 0.3),
         (40, 2, 5, 0, 0.0), (1100, 1, 3, 7, 0.0)]
FOCAL_TILE = 1024                             # OS_FOCAL_TILE of obstaclestats.hip


@pytest.mark.parametrize('N,S,T,O,bad', CASES)
def test_random_slices_against_numpy(N, S, T, O, bad):
    from piml_amd.obstaclestats import obstacle_stats
    O = _tile() + 1 if O is None else O
    P, V, M, side = random_slices(S, T, N, seed=N + T)
    if N == 1:
        P[:], V[:], M[:] = [0.5, 0.25], [0.3, -0.2], 1.0       # the one agent is there, next to the one point
    obs = REF.random_obstacles(O, side, seed=O, bad=bad)
    Pt, Vt, Mt = _gpu(P, V, M)
    for kw in option_sets(S, T, N, side):
        st = obstacle_stats(Pt, Vt, Mt, obs, **kw)
        want = check_against_ref(st, P, V, M, obs, f'N={N} S={S} T={T} O={O} {sorted(kw)}', **kw)
        assert st.clear.sum() == want['n_items'] == st.min_ttc.sum() and st.swept.sum() <= st.steps.sum()
        if N > FOCAL_TILE:                                    # agents of the second round are counted
            assert (st.trk_frames[:, FOCAL_TILE:] > 0).any()
        # no output is vacuous where there are enough frames and points for contacts: at 0.8 agents per m^2 and radius 0.25,
        # about 0.16 a frame and point, and three frames of seven points have none
        if N >= 65 and S * T * O >= 800:
            for k in REF.OUTPUTS + REF.HISTS:
                assert getattr(st, k).sum() > 0, k
            assert (st.trk_min >= 0).any() and st.min_ttc[:, :-1].sum() > 0
        if O == 0:
            assert all((getattr(st, k) == (-1 if k == 'trk_min' else 0)).all() for k in REF.OUTPUTS)
    if N == 1:
        assert st.focal.sum() == T and st.steps.sum() == T - 1
    if bad:
        assert (~np.isfinite(obs).all(1)).sum() > 50


def test_a_whole_tile_of_invalid_points():
    """more than a tile of points whose first tile is all NaN / infinite (filtered while staging: a tile with no valid point),
    and a list with no valid point at all: only focal and steps count"""
    from piml_amd.obstaclestats import obstacle_stats
    tile = _tile()
    P, V, M, side = random_slices(2, 6, 65, seed=3)
    obs = REF.random_obstacles(tile + 300, side, seed=1)
    obs[:tile:2], obs[1:tile:2, 1] = np.nan, -np.inf
    Pt, Vt, Mt = _gpu(P, V, M)
    st = obstacle_stats(Pt, Vt, Mt, obs)
    want = check_against_ref(st, P, V, M, obs, 'first tile invalid')
    assert st.contact.sum() > 0 and st.hit.sum() > 0
    for n in (tile, 5):
        none = obstacle_stats(Pt, Vt, Mt, obs[:n])
        check_against_ref(none, P, V, M, obs[:n], f'{n} invalid points')
        assert np.array_equal(none.focal, st.focal) and np.array_equal(none.steps, st.steps) and none.focal.sum() > 0
        assert none.clear.sum() == 0 and none.min_ttc.sum() == 0 and (none.trk_min == -1).all() and none.tracks.sum() == 0


def test_analytic_scene_is_exact():
    """the hand-counted scene of test_obstaclestats.py on the device: hand counts == device == both restatements"""
    from piml_amd.obstaclestats import obstacle_stats
    P, V, M, obs, kw, hand = REF.analytic_scene()
    st = obstacle_stats(*_gpu(P, V, M), obs, **kw)
    ref = REF.obstacle_stats(P, V, M, obs, **kw)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS:
        assert np.array_equal(getattr(st, k), hand[k]), (k, getattr(st, k), hand[k])
        assert np.array_equal(ref[k], hand[k]) and np.array_equal(ref['f64'][k], hand[k]), k
    for k in REF.HISTS:
        assert np.array_equal(getattr(st, k), hand[k]), k
    assert st.hit_rate() == 0.2 and st.hit_track_fraction() == 0.2 and st.mean_clearance() == 0.7


def _bits_equal(a, b, names=None):
    from piml_amd.obstaclestats import ARRAYS
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names or ARRAYS)


def test_determinism_graph_members_and_point_order():
    from piml_amd import ops_metrics
    from piml_amd.obstaclestats import obstacle_stats
    S, T, N = 3, 20, 150
    P, V, M, side = random_slices(S, T, N, seed=11)
    obs = REF.random_obstacles(_tile() + 50, side, seed=2, bad=0.05)
    Pt, Vt, Mt = _gpu(P, V, M)
    kw = dict(frames=(2, T - 1), box=(0.0, side * 0.7, 0.0, side * 0.7), hit_radius=0.125)
    a, b = obstacle_stats(Pt, Vt, Mt, obs, **kw), obstacle_stats(Pt, Vt, Mt, obs, **kw)
    assert _bits_equal(a, b) and a.hit.sum() > 0 and a.contact.sum() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), obstacle_stats(Pt[m], Vt[m], Mt[m], obs, **kw)), m
    # minima and integer sums are order-free: a permutation of the points (across the tile edge too) changes nothing
    perm = np.random.default_rng(0).permutation(obs.shape[0])
    assert _bits_equal(a, obstacle_stats(Pt, Vt, Mt, obs[perm], **kw), REF.OUTPUTS + REF.HISTS)
    ot = torch.tensor(obs, device=DEV)
    args = (Pt, Vt, Mt, ot, 0.08, 0.25, 0.125, 0.05, 100, 0.1, 100, kw['box'], kw['frames'], None)
    eager = ops_metrics.obstacle_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.obstacle_stats_frames(*args)                # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.obstacle_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


def test_recorded_clips():
    """the GC clip against its own obstacle points, whole; the UCY clip carries none (the loader's far-away placeholder), so
    it is taken against the GC scene's 4094 points, over a window that keeps the restatement quick"""
    from piml_amd.obstaclestats import compare_obstacle_stats, obstacle_stats_of_raw
    from piml_amd.scenarios import gc_scenario
    gc_obs = gc_scenario().obstacles.numpy()
    out = {}
    for name, obs, frames in ((GC_CLIP, None, None), (UCY_CLIP, gc_obs, (100, 250))):
        raw = _raw(name)
        P, V, M = (x.numpy() for x in (raw.position, raw.velocity, raw.mask_p))
        st = obstacle_stats_of_raw(raw, obs, frames=frames)
        assert st.options['dt'] == float(raw.time_unit)
        own = raw.obstacles.numpy() if obs is None else obs
        assert st.options['n_obstacles'] == own.shape[0]
        check_against_ref(st, P, V, M, own, name, frames=frames)
        assert st.focal.sum() > 0 and st.clear.sum() == st.focal.sum() and st.steps.sum() > 0
        out[name] = st
        print(f'[obstaclestats] {name}: mean clearance {st.mean_clearance():.3f} m, contact rate {st.contact_rate():.4g}, '
              f'hit rate {st.hit_rate():.4g}, tracks hit {st.hit_track_fraction():.4f}')
    with pytest.raises(ValueError):                            # different obstacle sets do not compare
        compare_obstacle_stats(out[GC_CLIP], out[UCY_CLIP])


@pytest.fixture(scope='module')
def gc_ensemble():
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    from piml_amd.simulate import load_mlapm_params
    return MLAPM(**load_mlapm_params(None)).simulate_ensemble(gc_scenario().to(DEV), FRAMES, SEEDS)


def test_short_ensemble_against_members_and_numpy(gc_ensemble):
    from piml_amd.obstaclestats import ADDITIVE, obstacle_stats_of_raw
    from piml_amd.scenarios import SCENARIOS
    ens = gc_ensemble
    st = ens.obstacle_stats()
    assert st.members == len(SEEDS) and st.options['dt'] == float(ens.time_unit) and st.options['n_obstacles'] == 4094
    assert st.focal.sum() > 0 and st.steps.sum() > 0 and st.clear.sum() == st.focal.sum()
    for m in range(len(SEEDS)):
        mem = ens.member(m)
        one = mem.obstacle_stats()
        assert _bits_equal(st.member(m), one), m
        raw = obstacle_stats_of_raw(mem.to_raw_data())          # the clip holds the member's num_agents slots only
        n = mem.num_agents
        assert _bits_equal(one, raw, ADDITIVE), m
        for k in REF.TRACK_ROWS:
            assert np.array_equal(getattr(one, k)[:, :n], getattr(raw, k)), (m, k)
    cap = ens.position.shape[2]
    check_against_ref(st, ens.position.cpu().numpy(), ens.velocity.cpu().numpy(), ens.mask_p.cpu().numpy(),
                      ens.obstacles.cpu().numpy(), 'MLAPM GC ensemble', n_active=[min(n, cap) for n in ens.spawned],
                      dt=float(ens.time_unit))
    with pytest.raises(ValueError, match='no obstacles'):
        from piml_amd.models.mlapm import MLAPM
        from piml_amd.simulate import load_mlapm_params
        MLAPM(**load_mlapm_params(None)).simulate_scenario(SCENARIOS['crosswalk']().to(DEV), 3).obstacle_stats()


def test_mlapm_hits_walls_at_least_as_often_as_the_recorded_crowd(gc_ensemble):
    """direction only: the law has no obstacle term, so over the same scene, obstacle points and frames its share of tracks
    that cross an obstacle is no smaller than the recorded GC clip's"""
    from piml_amd.obstaclestats import compare_obstacle_stats, obstacle_stats_of_raw
    sim = gc_ensemble.obstacle_stats()
    rec = obstacle_stats_of_raw(_raw(GC_CLIP), gc_ensemble.obstacles, frames=(0, FRAMES))
    whole = obstacle_stats_of_raw(_raw(GC_CLIP), gc_ensemble.obstacles)
    print(f'\n[obstaclestats] GC, seeds {SEEDS} x {FRAMES} frames: MLAPM hit_track_fraction {sim.hit_track_fraction():.4f} '
          f'(contact {sim.contact_track_fraction():.4f}, hit rate {sim.hit_rate():.4g}) against the recorded clip\'s '
          f'{rec.hit_track_fraction():.4f} (contact {rec.contact_track_fraction():.4f}, hit rate {rec.hit_rate():.4g}) over '
          f'the same frames; the whole recorded clip: {whole.hit_track_fraction():.4f} '
          f'(contact {whole.contact_track_fraction():.4f}, hit rate {whole.hit_rate():.4g})')
    assert sim.hit_track_fraction() >= rec.hit_track_fraction()
    c = compare_obstacle_stats(sim, rec)
    assert c['hit_track_fraction_diff'] >= 0 and np.isfinite(c['clearance_l1'])


def test_command_lines(tmp_path, gc_ensemble):
    """`simulate --obstacle-stats` and `python -m piml_amd.obstaclestats --data ... --ref ...` in child processes write what
    the Python calls return"""
    from piml_amd.crowdstats import _load
    from piml_amd.obstaclestats import ADDITIVE, ObstacleStats, merge, obstacle_stats_of_raw
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'walls.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scenario', 'gc', '--seeds', '0:3',
                        '--frames', str(FRAMES), '--out', clip, '--obstacle-stats', out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = ObstacleStats.from_json(out)
    own = gc_ensemble.obstacle_stats()
    assert _bits_equal(st, own), 'the JSON of the command line differs from the in-process statistics'
    assert st.options == own.options and not os.path.exists(clip.replace('{seed}', '0'))
    assert '[obstaclestats] simulate --obstacle-stats' in p.stdout
    # the stand-alone command on clips the ensemble wrote, against the recorded clip, all on the first clip's obstacles
    paths = gc_ensemble.save_data(clip)
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    cli = str(tmp_path / 'cli.json')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.obstaclestats', '--data', *paths, '--ref', ref, '--obstacles', paths[0],
                        '--frames', f'0:{FRAMES}', '--out', cli], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(cli) as fh:
        d = json.load(fh)
    data, rs = ObstacleStats.from_json(d['data']), ObstacleStats.from_json(d['ref'])
    obs = _load(paths[0]).obstacles
    assert data.trk_min is None and rs.trk_min is not None and data.options['n_obstacles'] == 4094
    assert _bits_equal(data, merge([obstacle_stats_of_raw(_load(q), obs, frames=(0, FRAMES)) for q in paths]), ADDITIVE)
    assert _bits_equal(rs, obstacle_stats_of_raw(_load(ref), obs, frames=(0, FRAMES)))
    assert set(d['compare']) >= {'clearance_l1', 'min_ttc_l1', 'track_min_clearance_l1', 'hit_rate_diff', 'speed_max_diff'}
    assert 'data vs ref' in p.stdout and 'mean clearance' in p.stdout
