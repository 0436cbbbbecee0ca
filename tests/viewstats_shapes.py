"""The inputs of test_viewstats_gpu.py and what test_viewstats.py checks of them without a GPU.

How many consecutive slices a workgroup of view_stats_kernel takes (its `run`), restated from the host code of
piml_amd/csrc/viewstats.hip with the constants (VS_TARGET_WG, VS_MAX_RUN, VS_MAX_GRID, VS_TILE) read out of the source: a
retune of a constant changes what these functions return, so the shapes' preconditions (asserted in both test files) fail
instead of the tests quietly going back to run = 1.  A slice is one (member, lag, frame), numbered member-major, then by
lag, as in pairstats.hip; a run is `run` consecutive slice numbers starting at a multiple of `run`.

The random cases, their option sets and the recorded clips, with the float64 restatement of each made once per process."""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'piml_amd', 'csrc')
CAP = 1e-3                                    # the ambiguous share a reference may report, as the other families'


@functools.lru_cache(maxsize=None)
def constant(name):
    """the value of `constexpr <integer type> name = <int> [<< <int>];` in viewstats.hip"""
    with open(os.path.join(CSRC, 'viewstats.hip')) as fh:
        text = fh.read()
    found = re.findall(r'constexpr\s+(?:long long|int)\s+' + re.escape(name) + r'\s*=\s*(\d+)\s*(?:<<\s*(\d+))?\s*;', text)
    if len(found) != 1:
        raise ValueError(f'{name}: {len(found)} definitions in viewstats.hip')
    base, shift = found[0]
    return int(base) << int(shift or 0)


def offsets(Tp, lags):
    """first slice of lag k within a member (lag 0 first; a lag at or past the window has no slices and shares the next
    offset), with the member's slice count last"""
    off = [0]
    for lag in (0,) + tuple(lags):
        off.append(off[-1] + max(Tp - lag, 0))
    return off


def run_of(S, Tp, lags):
    return min(max(S * offsets(Tp, lags)[-1] // constant('VS_TARGET_WG'), 1), constant('VS_MAX_RUN'))


def runs_of(S, Tp, lags):
    """the number of runs of the call: the workgroups it asks for before the grid cap"""
    return -(-S * offsets(Tp, lags)[-1] // run_of(S, Tp, lags))


def member_boundaries_inside_runs(S, Tp, lags):
    """the members 1 .. S - 1 whose first slice is not the first slice of a run"""
    run, pm = run_of(S, Tp, lags), offsets(Tp, lags)[-1]
    return [s for s in range(1, S) if (s * pm) % run != 0]


def lag_boundaries_inside_runs(S, Tp, lags):
    """(member, k) of the slices that start a lag k >= 1 (one with slices) in the middle of a run"""
    run, off = run_of(S, Tp, lags), offsets(Tp, lags)
    return [(s, k) for s in range(S) for k in range(1, len(off) - 1)
            if off[k + 1] > off[k] and (s * off[-1] + off[k]) % run != 0]


def run_one_group(Tp, lags):
    """the largest number of members whose call still has run == 1"""
    g = (2 * constant('VS_TARGET_WG') - 1) // offsets(Tp, lags)[-1]
    if g < 1 or run_of(g, Tp, lags) != 1:
        raise ValueError(f'no group of members of {offsets(Tp, lags)[-1]} slices has run == 1')
    return g


def check_run_shapes():
    """the preconditions of MID and LONG; a retune of the VS_* constants fails here"""
    for name, c in MID.items():
        assert run_of(c['S'], c['T'], c['lags']) == c['run'] == 3, (name, run_of(c['S'], c['T'], c['lags']))
        assert runs_of(c['S'], c['T'], c['lags']) < constant('VS_MAX_GRID')
        assert member_boundaries_inside_runs(c['S'], c['T'], c['lags']), name
        assert lag_boundaries_inside_runs(c['S'], c['T'], c['lags']), name
    c = LONG
    assert run_of(c['S'], c['T'], c['lags']) == c['run'] == constant('VS_MAX_RUN')
    assert member_boundaries_inside_runs(c['S'], c['T'], c['lags']) and lag_boundaries_inside_runs(c['S'], c['T'], c['lags'])
    assert run_one_group(c['T'], c['lags']) >= 1
    N, _, _ = CASES[0]
    assert N > constant('VS_TILE') + 256          # more than one source tile, more than one focal chunk in a tile


# ---------------------------------------------------------------------------------------------------------------------
# run = 3 against the restatement, run = VS_MAX_RUN against run = 1

WIDE = dict(cell=0.5, half=6, gap_bin=0.25, gap_bins=24)              # wide cells and bins: fewer pairs next to an edge
MID = {
    'base': dict(S=7, T=331, N=24, lags=(1, 7), run=3, seed=1),
    'empty_lag': dict(S=7, T=331, N=24, lags=(1, 7, 400), run=3, seed=1),
}
LONG = dict(S=150, T=300, N=6, lags=(1, 7, 400), run=64, seed=2)


def mid_n_active(S, N):
    """one member without a slot (every slice of it is empty), one with half the slots"""
    n = [N] * S
    n[2], n[4] = 0, N // 2
    return n


@functools.lru_cache(maxsize=None)
def mid_inputs(name):
    from test_flowstats_gpu import flow_slices
    c = MID[name]
    return flow_slices(c['S'], c['T'], c['N'], seed=c['seed'])


def mid_options(name, variant=None):
    c = MID[name]
    kw = dict(lags=c['lags'], **WIDE)
    if variant == 'n_active':
        kw['n_active'] = mid_n_active(c['S'], c['N'])
    return kw


@functools.lru_cache(maxsize=None)
def mid_reference(name, variant=None):
    import viewstats_ref
    P, V, M, _ = mid_inputs(name)
    return viewstats_ref.view_stats(P, V, M, **mid_options(name, variant))


MID_CALLS = (('base', None), ('empty_lag', None), ('base', 'n_active'))


# ---------------------------------------------------------------------------------------------------------------------
# the random slices of test_viewstats_gpu.py

# (1024 and 1025: a frame that just fills the staged tile and one that needs a second)
CASES = [(1500, 1, 4), (300, 3, 10), (65, 2, 6), (1, 1, 3), (1024, 2, 3), (1025, 2, 3)]
LAGS = (1, 2)


@functools.lru_cache(maxsize=None)
def case_inputs(N, S, T):
    """P, V, M, side from test_flowstats_gpu.flow_slices; callers leave them unchanged"""
    from test_flowstats_gpu import flow_slices
    return flow_slices(S, T, N, seed=N)


def option_sets(N, S, T):
    """the three option sets of a random case: defaults; box + window + r_max + a smaller, coarser map + fewer gap bins + a
    wider corridor; n_active per member, one member at 0 (the middle one; with one member only, a third of its slots) +
    the largest map + a narrower `with` / `against` cone"""
    side = case_inputs(N, S, T)[3]
    box = (0.1 * side, 0.6 * side, 0.2 * side, 0.9 * side)
    n_active = [N - (s * N) // (3 * S) for s in range(S)]
    if S > 1:
        n_active[S // 2] = 0
    else:
        n_active[0] = N - N // 3
    return (dict(lags=LAGS),
            dict(lags=LAGS, box=box, frames=(1, T), r_max=2.5, half=5, cell=0.4, gap_bins=20, corridor=0.8),
            dict(lags=LAGS, n_active=n_active, half=16, cos_same=0.9))


@functools.lru_cache(maxsize=None)
def case_reference(N, S, T, which):
    import viewstats_ref
    P, V, M, _ = case_inputs(N, S, T)
    return viewstats_ref.view_stats(P, V, M, **option_sets(N, S, T)[which])


# ---------------------------------------------------------------------------------------------------------------------
# the recorded clips

GC_CLIP = 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35'
UCY_CLIP = 'UCY_Dataset_time162-216_timeunit0.08'
GC_BOX = (5.0, 25.0, 15.0, 35.0)
CLIPS = ((GC_CLIP, GC_BOX), (UCY_CLIP, None))


@functools.lru_cache(maxsize=None)
def clip_arrays(name):
    from conftest import GOLDEN
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return tuple(np.ascontiguousarray(x.numpy()) for x in (raw.position, raw.velocity, raw.mask_p))


@functools.lru_cache(maxsize=None)
def clip_reference(name, box):
    import viewstats_ref
    return viewstats_ref.view_stats(*clip_arrays(name), box=box)


def ambiguous_share(want):
    return want['n_ambiguous'] / max(want['n_pairs'], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene: a focal agent at the origin walking +x at 1.3 m/s and five others, every value well inside its cell
# and bin for every agent in turn as the focal one, by 2 cm or more (defaults: cells of 0.25 m, X = 3 m, gap bins of 0.1 m,
# corridor 0.4 m)

SCENE_P = [[0.0, 0.0],        # 0: the focal agent
           [2.06, 0.29],      # 1: ahead, oncoming, slightly left
           [0.93, 0.17],      # 2: ahead in the corridor, same direction
           [1.77, -0.18],     # 3: ahead in the corridor, same direction
           [-1.28, 0.52],     # 4: behind, standing
           [0.34, -1.54]]     # 5: to the right, crossing (walking +y)
SCENE_V = [[1.3, 0.0], [-1.1, 0.0], [1.2, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 0.9]]


def rotate(xy):
    """(x, y) -> (-y, x): a quarter turn to the left, exact in float32"""
    xy = np.asarray(xy, np.float32)
    return np.stack([-xy[..., 1], xy[..., 0]], -1)
