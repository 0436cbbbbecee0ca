"""GPU: measurement-line statistics (piml_line_stats, piml_amd.linestats) against the numpy restatement (linestats_ref.py) on
random slices, the analytic scene and the recorded GC and UCY clips; determinism (two calls, graph replay, member against a
one-member call, a permutation of the lines, a reversed line), a short GC ensemble against its members and the two command
lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import linestats_ref as REF
from conftest import GOLDEN, REPO
from test_pairstats_gpu import GC_CLIP, UCY_CLIP, _gpu, _raw, random_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 1e-3                                    # the ambiguous share of items, as test_pairstats_gpu.py
Q = REF.Q
SEEDS, FRAMES = [0, 1, 2], 40                 # the short GC ensemble
GC_LINES = '0,2,30,2;2,5,2,17;28,7,28,26'       # 2 m inside the bottom, left and right entries of the GC hall


def check_against_ref(st, P, M, lines, label, **kw):
    want = REF.line_stats(P, M, lines, **kw)
    frac = want['n_ambiguous'] / max(want['n_items'], 1)
    print(f'\n[linestats] {label}: {want["n_items"]} items, {want["n_ambiguous"]} ambiguous ({frac:.2e})')
    assert frac <= CAP, frac                   # on the restatement alone, before the device is looked at
    dev = REF.check(st, want, label)
    print(f'[linestats] {label}: device == float32 run bit for bit: {all(v[0] == 0 for v in dev.values())}')
    return want


def option_sets(S, T, N):
    """the three option sets of a random case: defaults; window + n_active per member + other bin widths; one bin each"""
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    window = dict(frames=(1, T)) if T > 1 else {}
    return (dict(),
            dict(n_active=n_active, dt=0.1, v_bin=2.5, v_bins=12, w_bins=5, h_bin=0.02, h_bins=9, tt_bin=0.3, tt_bins=7, **window),
            dict(v_bin=20.0, v_bins=1, w_bins=1, h_bins=1, tt_bins=1))


CASES = [(1, 1, 1, 1), (1, 1, 2, 1), (65, 3, 40, 5), (300, 2, 12, 16), (3, 1, 600, 2)]     # N, S, T, L


@pytest.mark.parametrize('N,S,T,L', CASES)
def test_random_slices_against_numpy(N, S, T, L):
    from piml_amd.linestats import ARRAYS, line_stats
    P, _, M, side = random_slices(S, T, N, seed=N + T)
    lines = REF.random_lines(L, side, seed=L)
    if N == 1:
        P[:], M[:] = [0.25 * side, 0.5 * side], 1.0             # the one agent is there; with two frames it steps across
        P[:, -1, :, 0] = 0.75 * side
    Pt, Mt = _gpu(P, M)
    for kw in option_sets(S, T, N):
        st = line_stats(Pt, Mt, lines, **kw)
        want = check_against_ref(st, P, M, lines, f'N={N} S={S} T={T} L={L} {sorted(kw)}', **kw)
        assert np.array_equal(st.cross.sum(-1), st.trk_count.sum(-1))
        assert np.array_equal(st.nt.sum(-1), st.cross) and np.array_equal(st.speed.sum(-1), st.cross)
        assert np.array_equal(st.profile.sum(-1), st.cross) and (st.nt[..., -1] == 0).all()
        assert np.array_equal(st.trk_steps.sum(-1), st.steps) and st.steps.sum() * L == want['n_items']
        if N >= 65:
            for k in ARRAYS:                                    # no output is vacuous
                assert np.abs(getattr(st, k)).sum() > 0, k
            assert (st.trk_first >= 0).any() and (st.trk_dir == 0).any() and (st.trk_dir == 1).any()
    if N == 1:
        assert st.steps.sum() == T - 1 and st.cross.sum() == T - 1 and st.cross[0, 0, 1] == T - 1
        assert (st.trk_first[0, 0, 0] == Q // 2) if T == 2 else (st.trk_first == -1).all()
    if T == 600:
        assert (st.nt.sum((0, 1, 2)) > 0).sum() > 300            # crossings in every chunk of the window


def test_analytic_scene_is_exact():
    """the hand-counted scene of test_linestats.py on the device: hand counts == device == both restatements"""
    from piml_amd.linestats import line_stats
    P, M, lines, kw, hand = REF.analytic_scene()
    st = line_stats(*_gpu(P, M), lines, **kw)
    ref = REF.line_stats(P, M, lines, **kw)
    assert ref['n_ambiguous'] == 0
    for k in REF.OUTPUTS + REF.HISTS:
        assert np.array_equal(getattr(st, k), hand[k]), (k, getattr(st, k), hand[k])
        assert np.array_equal(ref[k], hand[k]) and np.array_equal(ref['f64'][k], hand[k]), k
    assert np.array_equal(st.flow(), hand['cross'][0] / 7.0)
    assert st.mean_headway()[0].tolist() == [1.75, 2.0 / 3] and st.mean_headway()[1, 1] == 1.5
    assert st.mean_travel_time()[0, 1] == 3.5 and np.isnan(st.mean_travel_time()[1, 0])
    # a reversed line swaps the two directions and mirrors the profile -- exactly here, where no crossing sits on a w bin edge.
    # The walkers whose count rests on a tie rule are left out, since the rules are not symmetric under the reversal: G, whose
    # crossing is at w = 0 of line 3 (w = 1 of its reverse), and E and F, who stand exactly on line 0 (the left side, which
    # the reversal moves to the other side)
    M2 = M.copy()
    M2[0, :, [REF.E, REF.F, REF.G]] = 0
    fwd = line_stats(*_gpu(P, M2), lines, **kw)
    rev = line_stats(*_gpu(P, M2), lines[:, [2, 3, 0, 1]], **kw)
    for k in ('cross', 'nt', 'speed', 'speed_sum', 'headway', 'headway_n', 'headway_sum'):
        assert np.array_equal(getattr(rev, k), getattr(fwd, k)[:, :, ::-1]), k
    assert np.array_equal(rev.profile, fwd.profile[:, :, ::-1, ::-1]) and fwd.profile.sum() == 9
    for k in ('trk_count', 'trk_first', 'travel', 'travel_n', 'travel_sum', 'steps', 'trk_steps'):
        assert np.array_equal(getattr(rev, k), getattr(fwd, k)), k
    assert np.array_equal(rev.trk_dir, np.where(fwd.trk_dir >= 0, 1 - fwd.trk_dir, -1))


def _bits_equal(a, b, names=None):
    from piml_amd.linestats import ARRAYS
    return all((getattr(a, k) is None and getattr(b, k) is None) or np.array_equal(getattr(a, k), getattr(b, k))
               for k in names or ARRAYS)


def test_determinism_graph_members_and_line_order():
    from piml_amd import ops_metrics
    from piml_amd.linestats import line_stats
    S, T, N, L = 3, 70, 150, 6
    P, _, M, side = random_slices(S, T, N, seed=11)
    lines = REF.random_lines(L, side, seed=3)
    Pt, Mt = _gpu(P, M)
    kw = dict(frames=(2, T - 1), v_bin=1.5, w_bins=7)
    a, b = line_stats(Pt, Mt, lines, **kw), line_stats(Pt, Mt, lines, **kw)
    assert _bits_equal(a, b) and a.cross.min() > 0
    for m in range(S):
        assert _bits_equal(a.member(m), line_stats(Pt[m], Mt[m], lines, **kw)), m
    # a permutation of the lines permutes the outputs
    perm = np.random.default_rng(0).permutation(L)
    c = line_stats(Pt, Mt, lines[perm], **kw)
    for k in ('cross', 'nt', 'speed', 'speed_sum', 'profile', 'trk_count', 'trk_first', 'trk_dir', 'headway', 'headway_n',
              'headway_sum'):
        assert np.array_equal(getattr(c, k), getattr(a, k)[:, perm]), k
    for k in ('travel', 'travel_n', 'travel_sum'):
        assert np.array_equal(getattr(c, k), getattr(a, k)[:, perm][:, :, perm]), k
    assert np.array_equal(c.steps, a.steps) and np.array_equal(c.trk_steps, a.trk_steps)
    # a reversed line swaps the directions; the profile is mirrored up to the crossings on a bin edge (w -> 1 - w rounds)
    r = line_stats(Pt, Mt, lines[:, [2, 3, 0, 1]], **kw)
    interior = (a.cross - r.cross[:, :, ::-1])
    print(f'\n[linestats] reversed lines: {int(np.abs(interior).sum())} of {int(a.cross.sum())} crossings at an end point')
    assert np.abs(interior).sum() <= 2 and np.abs(a.profile - r.profile[:, :, ::-1, ::-1]).sum() <= 8
    lt = torch.tensor(lines, device=DEV)
    args = (Pt, Mt, lt, 0.08, 1.5, 40, 7, kw['frames'], None)
    eager = ops_metrics.line_stats_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.line_stats_frames(*args)                     # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.line_stats_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, cap[k]), k
        assert np.array_equal(v.cpu().numpy(), getattr(a, k)), k


def test_recorded_clips():
    """the GC and UCY clips across the two mid-lines of their bounding boxes, whole"""
    from piml_amd.crowdstats import auto_box
    from piml_amd.linestats import auto_lines, line_stats_of_raw
    for name in (GC_CLIP, UCY_CLIP):
        raw = _raw(name)
        P, M = raw.position.numpy(), raw.mask_p.numpy()
        lines = auto_lines(auto_box(P, M, 0.5))
        st = line_stats_of_raw(raw, lines)
        assert st.options['dt'] == float(raw.time_unit) and st.n_lines == 2
        check_against_ref(st, P, M, lines, name, dt=float(raw.time_unit))
        assert st.cross.sum(-1).min() > 0 and st.steps.sum() > 0 and np.array_equal(st.cross.sum(-1), st.trk_count.sum(-1))
        print(f'[linestats] {name}: lines {lines.tolist()}, flow {st.flow().round(4).tolist()} /s, specific flow '
              f'{st.specific_flow().round(4).tolist()} /s/m, OD counts {st.od_counts().tolist()}, mean travel time '
              f'{np.round(st.mean_travel_time(), 2).tolist()} s, mean headway {st.mean_headway().round(3).tolist()} s')


@pytest.fixture(scope='module')
def gc_ensemble():
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    from piml_amd.simulate import load_mlapm_params
    return MLAPM(**load_mlapm_params(None)).simulate_ensemble(gc_scenario().to(DEV), FRAMES, SEEDS)


def _gc_lines():
    from piml_amd.linestats import parse_lines
    return parse_lines(GC_LINES)


def test_short_ensemble_against_members_and_numpy(gc_ensemble):
    from piml_amd.linestats import ADDITIVE, line_stats_of_raw
    ens, lines = gc_ensemble, _gc_lines()
    st = ens.line_stats(lines)
    assert st.members == len(SEEDS) and st.options['dt'] == float(ens.time_unit) and st.options['n_lines'] == 3
    assert st.steps.sum() > 0 and st.cross.sum() > 0 and (st.slices == FRAMES).all()
    for m in range(len(SEEDS)):
        mem = ens.member(m)
        one = mem.line_stats(lines)
        assert _bits_equal(st.member(m), one), m
        raw = line_stats_of_raw(mem.to_raw_data(), lines)       # the clip holds the member's num_agents slots only
        n = mem.num_agents
        assert _bits_equal(one, raw, ADDITIVE), m
        assert np.array_equal(one.trk_steps[:, :n], raw.trk_steps)
        for k in ('trk_count', 'trk_first', 'trk_dir'):
            assert np.array_equal(getattr(one, k)[:, :, :n], getattr(raw, k)), (m, k)
    cap = ens.position.shape[2]
    check_against_ref(st, ens.position.cpu().numpy(), ens.mask_p.cpu().numpy(), lines, 'MLAPM GC ensemble',
                      n_active=[min(n, cap) for n in ens.spawned], dt=float(ens.time_unit))


def test_command_lines(tmp_path, gc_ensemble):
    """`simulate --line-stats --lines` and `python -m piml_amd.linestats --data ... --ref ...` in child processes write what
    the Python calls return"""
    from piml_amd.crowdstats import _load, auto_box
    from piml_amd.linestats import ADDITIVE, LineStats, auto_lines, line_stats_of_raw, merge
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'lines.json')
    clip = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--scenario', 'gc', '--seeds', '0:3',
                        '--frames', str(FRAMES), '--out', clip, '--line-stats', out, '--lines', GC_LINES], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    st = LineStats.from_json(out)
    own = gc_ensemble.line_stats(_gc_lines())
    assert _bits_equal(st, own), 'the JSON of the command line differs from the in-process statistics'
    assert st.options == own.options and not os.path.exists(clip.replace('{seed}', '0'))
    assert '[linestats] simulate --line-stats' in p.stdout
    # the stand-alone command on clips the ensemble wrote, against the recorded clip, on the mid-lines of the recorded clip's box
    paths = gc_ensemble.save_data(clip)
    ref = os.path.join(GOLDEN, 'data', GC_CLIP + '.npy')
    cli = str(tmp_path / 'cli.json')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.linestats', '--data', *paths, '--ref', ref, '--lines', 'auto', '--box',
                        'auto', '--frames', f'0:{FRAMES}', '--out', cli], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    with open(cli) as fh:
        d = json.load(fh)
    data, rs = LineStats.from_json(d['data']), LineStats.from_json(d['ref'])
    rec = _load(ref)
    lines = auto_lines(auto_box(rec.position.numpy(), rec.mask_p.numpy(), 0.5))
    assert data.trk_first is None and rs.trk_first is not None and data.options['lines_hash'] == rs.options['lines_hash']
    assert _bits_equal(data, merge([line_stats_of_raw(_load(q), lines, frames=(0, FRAMES)) for q in paths]), ADDITIVE)
    assert _bits_equal(rs, line_stats_of_raw(rec, lines, frames=(0, FRAMES)))
    assert set(d['compare']) >= {'flow_rel_diff', 'direction_split_diff', 'speed_l1', 'profile_l1', 'headway_l1', 'travel_l1',
                                 'mean_travel_rel_diff'}
    assert 'data vs ref' in p.stdout and '--box auto' in p.stdout and 'crossings' in p.stdout
