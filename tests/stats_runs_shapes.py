"""How many consecutive slices a workgroup of pair_stats_kernel, flow_stats_kernel and obstacle_stats_kernel takes (its
`run`) for a given call, restated from the host code of piml_amd/csrc/{pairstats,flowstats,obstaclestats}.hip with the
constants (*_TARGET_WG, *_MAX_RUN, *_MAX_GRID) read out of the sources, and the shapes test_stats_runs_gpu.py and
test_stats_grid_cap_gpu.py use.  A retune of a constant changes what these functions return, so the shapes' preconditions
(test_stats_runs_shapes.py, and again inside the GPU tests) fail instead of the tests quietly going back to run = 1.

A slice is one (member, frame) -- for pairs one (member, lag, frame) -- and slices are numbered member-major; a run is
`run` consecutive slice numbers starting at a multiple of `run`."""
import functools
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'piml_amd', 'csrc')
SOURCES = {'PS': 'pairstats.hip', 'FS': 'flowstats.hip', 'OS': 'obstaclestats.hip', 'TS': 'trackstats.hip',
           'CD': 'crowdstats.hpp'}


@functools.lru_cache(maxsize=None)
def constant(name):
    """the value of `constexpr <integer type> name = <int> [<< <int>];` in the source its prefix names"""
    path = os.path.join(CSRC, SOURCES[name.split('_')[0]])
    with open(path) as fh:
        text = fh.read()
    found = re.findall(r'constexpr\s+(?:long long|int|unsigned)\s+' + re.escape(name) + r'\s*=\s*(\d+)\s*(?:<<\s*(\d+))?\s*;',
                       text)
    if len(found) != 1:
        raise ValueError(f'{name}: {len(found)} definitions in {path}')
    base, shift = found[0]
    return int(base) << int(shift or 0)


def _run(prefix, slices):
    return min(max(slices // constant(prefix + '_TARGET_WG'), 1), constant(prefix + '_MAX_RUN'))


def pair_offsets(Tp, lags):
    """first slice of lag k within a member (lag 0 first; a lag at or past the window has no slices and shares the next
    offset), with the member's slice count last"""
    off = [0]
    for lag in (0,) + tuple(lags):
        off.append(off[-1] + max(Tp - lag, 0))
    return off


def pair_run(S, Tp, lags):
    return _run('PS', S * pair_offsets(Tp, lags)[-1])


def flow_run(S, Tp):
    return _run('FS', S * Tp)


def obstacle_run(S, Tp):
    return _run('OS', S * Tp)


RUN = {'pairs': pair_run, 'flow': lambda S, Tp, lags=(): flow_run(S, Tp),
       'obstacles': lambda S, Tp, lags=(): obstacle_run(S, Tp)}
PREFIX = {'pairs': 'PS', 'flow': 'FS', 'obstacles': 'OS'}


def per_member(kind, Tp, lags=()):
    return pair_offsets(Tp, lags)[-1] if kind == 'pairs' else Tp


def run_of(kind, S, Tp, lags=()):
    return RUN[kind](S, Tp, lags)


def runs_of(kind, S, Tp, lags=()):
    """the number of runs of the call: the workgroups it asks for before the grid cap"""
    run = run_of(kind, S, Tp, lags)
    return -(-S * per_member(kind, Tp, lags) // run)


def member_boundaries_inside_runs(kind, S, Tp, lags=()):
    """the members 1 .. S - 1 whose first slice is not the first slice of a run: the workgroup that takes it has the
    previous member's counts in its accumulator"""
    run, pm = run_of(kind, S, Tp, lags), per_member(kind, Tp, lags)
    return [s for s in range(1, S) if (s * pm) % run != 0]


def lag_boundaries_inside_runs(S, Tp, lags):
    """(member, k) of the pair slices that start a lag k >= 1 (one with slices) in the middle of a run"""
    run, off = pair_run(S, Tp, lags), pair_offsets(Tp, lags)
    return [(s, k) for s in range(S) for k in range(1, len(off) - 1)
            if off[k + 1] > off[k] and (s * off[-1] + off[k]) % run != 0]


def run_one_group(kind, Tp, lags=()):
    """the largest number of members whose call still has run == 1"""
    g = (2 * constant(PREFIX[kind] + '_TARGET_WG') - 1) // per_member(kind, Tp, lags)
    if g < 1 or run_of(kind, g, Tp, lags) != 1:
        raise ValueError(f'{kind}: no group of members of {per_member(kind, Tp, lags)} slices has run == 1')
    return g


# ---------------------------------------------------------------------------------------------------------------------
# the shapes of test_stats_runs_gpu.py: run = 3 against the float64 restatements, run = 64 against run = 1

PAIR_BINS = dict(r_bin=0.25, r_bins=20, tau_bin=0.2, tau_bins=25)      # wide bins: fewer pairs next to an edge
MID = {
    'pairs': dict(S=7, T=331, N=24, lags=(1, 7), run=3, seed=1),
    'pairs_empty_lag': dict(S=7, T=331, N=24, lags=(1, 7, 400), run=3, seed=1),
    'flow': dict(S=9, T=701, N=24, lags=(), run=3, seed=1),
    'obstacles': dict(S=13, T=950, N=16, lags=(), run=3, seed=1, O=7),
}
LONG = {
    'pairs': dict(S=150, T=300, N=6, lags=(1, 7, 400), run=64, seed=2),
    'flow': dict(S=150, T=900, N=6, lags=(), run=64, seed=2),
    'obstacles': dict(S=300, T=900, N=4, lags=(), run=64, seed=2, O=7),
}
FLOW_BOX = (0.1, 0.9, 0.1, 0.9)               # times the side of the square
CAP = 1e-3                                    # the ambiguous share a reference may report, as test_pairstats_gpu.py


def kind_of(name):
    return name.split('_')[0]


def pair_n_active(S, N):
    """one member without a slot (every slice of it is empty), one with half the slots"""
    n = [N] * S
    n[2], n[4] = 0, N // 2
    return n


# the shapes of test_stats_grid_cap_gpu.py: more workgroups than the grid cap, so that some take a second item
TRACKS = dict(S=17, T=4, N=65536, n_lags=2, halves=((0, 9), (9, 17)))
CROWD = dict(S=3, T=350000, N=2, rho_bins=3)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references of the mid-size cases, made once per process

@functools.lru_cache(maxsize=None)
def mid_inputs(name):
    """P, V, M, side of a mid-size case, from the generators of the run = 1 tests; callers leave them unchanged"""
    c = MID[name]
    if kind_of(name) == 'flow':
        from test_flowstats_gpu import flow_slices
        return flow_slices(c['S'], c['T'], c['N'], seed=c['seed'])
    from test_pairstats_gpu import random_slices
    return random_slices(c['S'], c['T'], c['N'], seed=c['seed'])


def mid_options(name, variant=None):
    """the keywords of the device call and of the restatement alike"""
    c = MID[name]
    if kind_of(name) == 'pairs':
        kw = dict(lags=c['lags'], **PAIR_BINS)
        if variant == 'n_active':
            kw['n_active'] = pair_n_active(c['S'], c['N'])
        return kw
    if kind_of(name) == 'flow':
        side = mid_inputs(name)[3]
        return dict(box=tuple(float(f * side) for f in FLOW_BOX))
    return {}


def mid_obstacles(name, variant=None, tile=None):
    import obstaclestats_ref
    side = mid_inputs(name)[3]
    O = MID[name]['O'] if variant is None else tile + 300
    return obstaclestats_ref.random_obstacles(O, side, seed=O)


@functools.lru_cache(maxsize=None)
def mid_reference(name, variant=None, tile=None):
    """the float64 restatement of a mid-size case (variant: None, 'n_active' for pairs, 'tiles' with the tile size for
    obstacles); callers leave it unchanged"""
    P, V, M, _ = mid_inputs(name)
    kw = mid_options(name, variant)
    if kind_of(name) == 'pairs':
        import pairstats_ref
        return pairstats_ref.pair_stats(P, V, M, **kw)
    if kind_of(name) == 'flow':
        import flowstats_ref
        return flowstats_ref.flow_stats(P, V, M, **kw)
    import obstaclestats_ref
    return obstaclestats_ref.obstacle_stats(P, V, M, mid_obstacles(name, variant, tile), **kw)


def ambiguous_share(kind, want):
    return want['n_ambiguous'] / max(want['n_items' if kind == 'obstacles' else 'n_pairs'], 1)
