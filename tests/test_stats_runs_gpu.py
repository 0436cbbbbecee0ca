"""GPU: pair_stats_kernel, flow_stats_kernel and obstacle_stats_kernel where a workgroup takes a run of consecutive slices
(the path of every real calibration: tens of members x hundreds of frames), which no other test reaches -- there every
comparison has run == 1.  Run = 3 against the float64 restatements, with member boundaries, lag boundaries, a lag without
slices, empty slices and each member's last frame in the middle of runs; run = 64 (the cap) bit for bit against the same
members taken in groups small enough for run == 1, which the run = 1 tests hold against numpy, and bit for bit again on a
second call and a graph replay.  The shapes and their preconditions are in stats_runs_shapes.py (checked on the CPU by
test_stats_runs_shapes.py and again here, so that a retune of a constant fails loudly)."""
import time

import numpy as np
import pytest
import torch

import flowstats_ref
import obstaclestats_ref
import pairstats_ref
import stats_runs_shapes as SH
from test_flowstats_gpu import flow_slices
from test_obstaclestats_gpu import _tile
from test_pairstats_gpu import _gpu, random_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _precondition(kind, c):
    """the run the case was chosen for, with a member boundary strictly inside a run"""
    S, T, lags = c['S'], c['T'], c['lags']
    assert SH.run_of(kind, S, T, lags) == c['run'] and SH.per_member(kind, T, lags) % c['run'] != 0
    assert SH.member_boundaries_inside_runs(kind, S, T, lags)
    if kind == 'pairs':
        assert {k for _, k in SH.lag_boundaries_inside_runs(S, T, lags)} == {1, 2}


def _distinct(rows):
    """no two members share a row: a flush to the wrong member cannot cancel"""
    return len({np.ascontiguousarray(r).tobytes() for r in rows}) == len(rows)


def _timed(fn, *a, **kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


# ---------------------------------------------------------------------------------------------------------------------
# run = 3 against the float64 restatements

@pytest.mark.parametrize('name,variant', [('pairs', None), ('pairs_empty_lag', None), ('pairs', 'n_active')])
def test_pairs_run3_against_numpy(name, variant):
    from piml_amd.pairstats import pair_stats
    c = SH.MID[name]
    _precondition('pairs', c)
    P, V, M, _ = SH.mid_inputs(name)
    kw = SH.mid_options(name, variant)
    st, sec = _timed(pair_stats, *_gpu(P, V, M), **kw)
    want = SH.mid_reference(name, variant)
    share = SH.ambiguous_share('pairs', want)
    print(f'\n[stats runs] {name} {variant}: run {c["run"]}, {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous '
          f'({share:.2e}); device call {sec * 1e3:.1f} ms')
    assert share <= SH.CAP, share
    pairstats_ref.check(st, want, f'{name} {variant}')
    bound = kw.get('n_active', [c['N']] * c['S'])
    full = [s for s in range(c['S']) if bound[s] >= 2]
    for s in full:                                               # no member's statistics are vacuous, at any lag with slices
        for k in (0, 1, 2):
            assert st.focal[s, k] > 0 and st.ttc[s, k].sum() > 0 and st.overlap[s, k] > 0 and st.dist[s, k].sum() > 0, (s, k)
        assert st.nn[s].sum() == st.focal[s, 0] == st.min_ttc[s].sum() and st.min_ttc[s, :-1].sum() > 0
        assert _distinct([st.ttc[s, k] for k in (0, 1, 2)]), s   # nor do its lags share a row
    for k in ('ttc', 'dist', 'nn', 'min_ttc'):
        assert _distinct([getattr(st, k)[s] for s in full]), k
    if len(c['lags']) == 3:                                      # the lag past the window: no slices, zero counts
        assert all((getattr(st, k)[:, 3] == 0).all() for k in ('focal', 'pairs', 'overlap', 'ttc', 'dist'))
    if variant == 'n_active':
        empty = [s for s in range(c['S']) if bound[s] == 0]
        assert len(empty) == 1 and len(full) == c['S'] - 1
        assert all((getattr(st, k)[empty[0]] == 0).all() for k in pairstats_ref.OUTPUTS)
        assert st.focal[4, 0] < st.focal[3, 0] * 0.7             # half the slots


def test_flow_run3_against_numpy():
    from piml_amd.flowstats import flow_stats
    c = SH.MID['flow']
    _precondition('flow', c)
    P, V, M, _ = SH.mid_inputs('flow')
    kw = SH.mid_options('flow')
    st, sec = _timed(flow_stats, *_gpu(P, V, M), **kw)
    want = SH.mid_reference('flow')
    share = SH.ambiguous_share('flow', want)
    print(f'\n[stats runs] flow: run {c["run"]}, {want["n_pairs"]} pairs, {want["n_ambiguous"]} ambiguous ({share:.2e}); '
          f'device call {sec * 1e3:.1f} ms')
    assert share <= SH.CAP, share
    flowstats_ref.check(st, want, 'flow run 3')                  # the per-member rows, the six per-slice series and the map
    assert all(getattr(st, k).shape == (c['S'], c['T']) for k in flowstats_ref.SERIES) and st.map_n is not None
    for s in range(c['S']):
        assert st.corr_pairs[s].sum() > 0 and st.corr_sum[s].any() and st.map_n[s].sum() > 0 and st.map_vx[s].any(), s
        for k in flowstats_ref.SERIES:
            assert getattr(st, k)[s].sum() > 0 and len(set(getattr(st, k)[s].tolist())) > 3, (s, k)
    for k in ('corr_pairs', 'corr_sum', 'map_n') + flowstats_ref.SERIES:
        assert _distinct(list(getattr(st, k))), k


def _obstacle_checks(st, S):
    for s in range(S):
        for k in obstaclestats_ref.OUTPUTS + obstaclestats_ref.HISTS:
            assert getattr(st, k)[s].sum() > 0, (s, k)
        assert st.min_ttc[s, :-1].sum() > 0
        # a member's last frame has no next one: were it taken for a step (it lies inside a run), steps would reach focal
        assert 0 < st.steps[s] < st.focal[s], s
    for k in ('clear', 'clear_speed', 'swept', 'min_ttc', 'trk_frames', 'trk_min'):
        assert _distinct(list(getattr(st, k))), k


def test_obstacles_run3_against_numpy():
    from piml_amd.obstaclestats import obstacle_stats
    c = SH.MID['obstacles']
    _precondition('obstacles', c)
    P, V, M, _ = SH.mid_inputs('obstacles')
    obs = SH.mid_obstacles('obstacles')
    assert obs.shape[0] == c['O'] <= _tile()
    st, sec = _timed(obstacle_stats, *_gpu(P, V, M), obs)
    want = SH.mid_reference('obstacles')
    share = SH.ambiguous_share('obstacles', want)
    print(f'\n[stats runs] obstacles: run {c["run"]}, {want["n_items"]} items, {want["n_ambiguous"]} ambiguous ({share:.2e}); '
          f'device call {sec * 1e3:.1f} ms')
    assert share <= SH.CAP, share
    obstaclestats_ref.check(st, want, 'obstacles run 3')
    _obstacle_checks(st, c['S'])
    # the frame before a member's last is a step for every agent there at both, the last is for none: by hand for member 0
    part = obstaclestats_ref.participants(P[0], V[0], M[0])
    assert st.steps[0] == (part[:-1] & part[1:]).sum() and part[-1].sum() > 0


def test_obstacles_run3_more_than_a_tile_of_points():
    """O = tile + 300: the points are staged again, tile by tile, in every slice of a run.  The restatement needs 33 s on
    the CPU for all 13 members of this shape (150,000 items x 4,396 points, twice), so it is taken for members 4 and 5 --
    both start inside a run, 4 x 950 % 3 = 2 and 5 x 950 % 3 = 1 -- and every member of the one call is compared bit for bit
    with the same members in groups of run == 1, the path test_obstaclestats_gpu.py holds against numpy with more than a
    tile."""
    from piml_amd.obstaclestats import obstacle_stats
    c = SH.MID['obstacles']
    _precondition('obstacles', c)
    tile = _tile()
    P, V, M, _ = SH.mid_inputs('obstacles')
    obs = SH.mid_obstacles('obstacles', 'tiles', tile)
    assert obs.shape[0] == tile + 300 and np.isfinite(obs).all()
    Pt, Vt, Mt = _gpu(P, V, M)
    st, sec = _timed(obstacle_stats, Pt, Vt, Mt, obs)
    print(f'\n[stats runs] obstacles, {obs.shape[0]} points: run {c["run"]}, device call {sec * 1e3:.1f} ms')
    _obstacle_checks(st, c['S'])
    names = obstaclestats_ref.OUTPUTS + obstaclestats_ref.HISTS
    g = SH.run_one_group('obstacles', c['T'])
    for a in range(0, c['S'], g):
        b = min(a + g, c['S'])
        assert SH.obstacle_run(b - a, c['T']) == 1
        part = obstacle_stats(Pt[a:b], Vt[a:b], Mt[a:b], obs)
        for k in names:
            assert np.array_equal(getattr(st, k)[a:b], getattr(part, k)), (k, a, b)
    pair = [4, 5]
    assert {4, 5} <= set(SH.member_boundaries_inside_runs('obstacles', c['S'], c['T']))
    want = obstaclestats_ref.obstacle_stats(P[pair], V[pair], M[pair], obs)
    share = SH.ambiguous_share('obstacles', want)
    print(f'[stats runs] obstacles, {obs.shape[0]} points, members {pair}: {want["n_items"]} items, {want["n_ambiguous"]} '
          f'ambiguous ({share:.2e})')
    assert share <= SH.CAP, share
    obstaclestats_ref.check({k: getattr(st, k)[pair] for k in obstaclestats_ref.OUTPUTS}, want, 'obstacles run 3, tiles')


# ---------------------------------------------------------------------------------------------------------------------
# run = 64 bit for bit against run = 1, a second call and a graph replay

def _in_groups(kind, c, call, names):
    """the members in groups of run == 1: every output laid member after member"""
    g = SH.run_one_group(kind, c['T'], c['lags'])
    parts = []
    for a in range(0, c['S'], g):
        b = min(a + g, c['S'])
        assert SH.run_of(kind, b - a, c['T'], c['lags']) == 1
        parts.append(call(a, b))
    return {k: None if getattr(parts[0], k) is None else np.concatenate([getattr(p, k) for p in parts], 0) for k in names}


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


def _same_bits(st, other, names, label):
    for k in names:
        x, y = getattr(st, k), other[k] if isinstance(other, dict) else getattr(other, k)
        assert (x is None and y is None) or np.array_equal(x, y), (label, k)


def _graph_bits(st, eager, cap, label):
    for k, v in eager.items():
        assert (v is None and cap[k] is None) or torch.equal(v, cap[k]), (label, k)
        assert v is None or np.array_equal(v.cpu().numpy(), getattr(st, k)), (label, k)


def test_pairs_run64_equals_run1_bit_for_bit():
    from piml_amd import ops_metrics
    from piml_amd.pairstats import pair_stats
    c = SH.LONG['pairs']
    _precondition('pairs', c)
    assert SH.constant('PS_MAX_RUN') == c['run']
    P, V, M, side = random_slices(c['S'], c['T'], c['N'], seed=c['seed'])
    Pt, Vt, Mt = _gpu(P, V, M)
    kw = dict(lags=c['lags'], box=(0.0, 0.8 * side, 0.0, 0.8 * side))
    st, sec = _timed(pair_stats, Pt, Vt, Mt, **kw)
    print(f'\n[stats runs] pairs: run {c["run"]}, {c["S"]} members, device call {sec * 1e3:.1f} ms')
    names = pairstats_ref.OUTPUTS
    for s in range(c['S']):
        assert all(st.ttc[s, k].sum() > 0 and st.overlap[s, k] > 0 for k in (0, 1, 2)) and st.focal[s, 3] == 0, s
    assert _distinct(list(st.dist)) and _distinct(list(st.nn))
    _same_bits(st, _in_groups('pairs', c, lambda a, b: pair_stats(Pt[a:b], Vt[a:b], Mt[a:b], **kw), names), names, 'groups')
    _same_bits(st, pair_stats(Pt, Vt, Mt, **kw), names, 'second call')
    _graph_bits(st, *_replayed(ops_metrics.pair_stats_frames, Pt, Vt, Mt, lags=c['lags'], box=kw['box']), 'graph')


def test_flow_run64_equals_run1_bit_for_bit():
    from piml_amd import ops_metrics
    from piml_amd.flowstats import flow_stats
    c = SH.LONG['flow']
    _precondition('flow', c)
    assert SH.constant('FS_MAX_RUN') == c['run']
    P, V, M, side = flow_slices(c['S'], c['T'], c['N'], seed=c['seed'])
    Pt, Vt, Mt = _gpu(P, V, M)
    box = tuple(float(f * side) for f in SH.FLOW_BOX)
    st, sec = _timed(flow_stats, Pt, Vt, Mt, box=box)
    print(f'\n[stats runs] flow: run {c["run"]}, {c["S"]} members, device call {sec * 1e3:.1f} ms')
    names = flowstats_ref.OUTPUTS                                # the rows, the six series and the three maps
    for s in range(c['S']):
        assert st.corr_pairs[s].sum() > 0 and st.lane_opp[s].sum() > 0 and st.lane_same[s].sum() > 0 \
            and st.map_n[s].sum() > 0, s
    assert _distinct(list(st.corr_pairs)) and _distinct(list(st.lane_n)) and _distinct(list(st.map_vx))
    _same_bits(st, _in_groups('flow', c, lambda a, b: flow_stats(Pt[a:b], Vt[a:b], Mt[a:b], box=box), names), names,
               'groups')
    _same_bits(st, flow_stats(Pt, Vt, Mt, box=box), names, 'second call')
    _graph_bits(st, *_replayed(ops_metrics.flow_stats_frames, Pt, Vt, Mt, box=box, grid=flowstats_ref.grid_shape(box, 0.5)),
                'graph')


def test_obstacles_run64_equals_run1_bit_for_bit():
    from piml_amd import ops_metrics
    from piml_amd.obstaclestats import obstacle_stats
    c = SH.LONG['obstacles']
    _precondition('obstacles', c)
    assert SH.constant('OS_MAX_RUN') == c['run']
    P, V, M, side = random_slices(c['S'], c['T'], c['N'], seed=c['seed'])
    obs = obstaclestats_ref.random_obstacles(c['O'], side, seed=c['O'])
    Pt, Vt, Mt = _gpu(P, V, M)
    st, sec = _timed(obstacle_stats, Pt, Vt, Mt, obs)
    print(f'\n[stats runs] obstacles: run {c["run"]}, {c["S"]} members, device call {sec * 1e3:.1f} ms')
    names = obstaclestats_ref.OUTPUTS + obstaclestats_ref.HISTS  # the counts, the rows, the per-track rows and their histograms
    for s in range(c['S']):
        assert st.contact[s] > 0 and st.hit[s] > 0 and 0 < st.steps[s] < st.focal[s] and st.min_ttc[s, :-1].sum() > 0, s
    assert _distinct(list(st.clear)) and _distinct(list(st.trk_min))
    _same_bits(st, _in_groups('obstacles', c, lambda a, b: obstacle_stats(Pt[a:b], Vt[a:b], Mt[a:b], obs), names), names,
               'groups')
    _same_bits(st, obstacle_stats(Pt, Vt, Mt, obs), names, 'second call')
    _graph_bits(st, *_replayed(ops_metrics.obstacle_stats_frames, Pt, Vt, Mt, torch.tensor(obs, device=DEV)), 'graph')
