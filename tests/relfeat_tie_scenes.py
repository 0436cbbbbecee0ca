"""Tie-rich scenes for the neighbour search (piml_amd/csrc/relfeat.hip: relfeat_fwd_kernel) and the launch form each one is meant to
reach, for test_relfeat_tie_scenes.py (CPU: the scenes' preconditions, by the oracle alone) and test_relfeat_ties_gpu.py.

Every coordinate is a multiple of 0.25, so the squared distances are exact in float32, equal distances are EXACTLY equal after the
square root, and the oracle's (distance, index) order has real ties in it: the lowest index wins, a source at the k-th distance
with a higher index stays out, one with a lower index displaces the k-th entry.  numpy only, seeded."""
import ctypes
import functools

import numpy as np

F32 = np.float32
SEED = 1
TILE = 4096          # kTile of relfeat.hip: source points per LDS tile
RING = 1024          # kRing: entries of a wave's candidate ring


def lattice(C, N, M, side, seed=SEED):
    """C slices of N agents on integers(0, side) * 0.5, M obstacle points on the same lattice shifted by 0.25; integer velocities
    (15 % zero: headings on the axes and diagonals, or none), 5 % of the agents absent (NaN position and destination), random
    accelerations with some NaN.  A leading slice axis is kept only for C > 1."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, side, size=(C, N, 2)).astype(F32) * F32(0.5)
    o = rng.integers(0, side, size=(M, 2)).astype(F32) * F32(0.5) + F32(0.25)
    v = np.round(rng.standard_normal((C, N, 2))).astype(F32)
    v[rng.random((C, N)) < 0.15] = 0
    a = (rng.standard_normal((C, N, 2)) * 0.3).astype(F32)
    a[rng.random((C, N)) < 0.05] = np.nan
    d = rng.integers(0, side, size=(C, N, 2)).astype(F32) * F32(0.5)
    absent = rng.random((C, N)) < 0.05
    p[absent] = np.nan
    d[absent] = np.nan
    v0 = (1.0 + rng.random((C, N, 1))).astype(F32)
    sc = dict(position=p, velocity=v, acceleration=a, destination=d, desired_speed=v0)
    if C == 1:
        sc = {k: x[0] for k, x in sc.items()}
    sc['obstacles'] = o
    return sc


PILE_TAIL = 8        # the last agents of a pile: 4 far away (they see themselves only), then 4 absent


def pile(N, M, seed=SEED):
    """Agents alternate between (0, 0) and (0, 0.5), all heading +x; three obstacle points in four lie on (1.25, 0.25) -- the same
    distance from both agent points -- the fourth on (1.75, 0.25).  For sight angles >= 100 a coincident source (cosine 0) is in
    view, so every row has about N / 2 sources at distance exactly 0 and 3 M / 4 obstacle points at one distance: far more than
    the ring holds.  The last PILE_TAIL agents are 4 loners out of everybody's range and 4 absent ones."""
    rng = np.random.default_rng(seed)
    i = np.arange(N)
    p = np.stack((np.zeros(N), 0.5 * (i % 2)), -1).astype(F32)
    p[N - 8:N - 4] = np.stack((np.full(4, 50.0), 10.0 * np.arange(4)), -1)
    v = np.tile(np.array([1, 0], F32), (N, 1))
    a = np.round(rng.standard_normal((N, 2))).astype(F32) * F32(0.25)
    d = p + np.array([5, 0], F32)
    p[N - 4:] = np.nan
    d[N - 4:] = np.nan
    j = np.arange(M)
    o = np.stack((np.where(j % 4 == 3, 1.75, 1.25), np.full(M, 0.25)), -1).astype(F32)
    return dict(position=p, velocity=v, acceleration=a, destination=d, desired_speed=np.full((N, 1), 1.25, F32), obstacles=o)


# name -> (builder, arguments).  The shapes are the smallest that reach the form (FORMS below): no case is larger than the hall.
SCENES = {
    'hall': (lattice, dict(C=1, N=4500, M=2500, side=40)),
    'hall_x2': (lattice, dict(C=2, N=4500, M=2500, side=40)),
    'edge_4096': (lattice, dict(C=1, N=4096, M=64, side=40)),
    'edge_4097': (lattice, dict(C=1, N=4097, M=64, side=40)),
    'obstacle_tiles': (lattice, dict(C=1, N=600, M=4500, side=40)),
    'slices': (lattice, dict(C=8, N=600, M=130, side=12)),
    'many_slices': (lattice, dict(C=32, N=520, M=64, side=10)),
    'small_600': (lattice, dict(C=1, N=600, M=130, side=24)),
    'small_1500': (lattice, dict(C=1, N=1500, M=130, side=24)),
    'lattice_9000': (lattice, dict(C=1, N=9000, M=300, side=56)),
    'pile': (pile, dict(N=3000, M=1500)),
}
DEFAULT_GEOM = dict(topk_ped=6, sight_angle_ped=90, dist_threshold_ped=4, topk_obs=10, sight_angle_obs=90, dist_threshold_obs=4)
GEOM = {'pile': dict(DEFAULT_GEOM, sight_angle_ped=180, sight_angle_obs=180)}
KMAX = dict(topk_ped=32, topk_obs=32)

# The form the dispatch rule of relfeat.hip (relfeat_plan) gives a one-launch call of the case:
# (waves, resident, split, agent tiles, obstacle tiles).  A retune moves these and the tests that assert them fail.
FORMS = {
    'hall': (8, 0, 1, 2, 1),
    'hall_x2': (8, 0, 0, 2, 1),                # unsplit, non-resident: both passes behind the workgroup's barriers
    'edge_4096': (16, 0, 1, 1, 1),
    'edge_4097': (8, 0, 1, 2, 1),              # one source in the second tile
    'obstacle_tiles': (4, 0, 1, 1, 2),
    'slices': (16, 1, 0, 1, 1),
    'many_slices': (8, 1, 0, 1, 1),            # rows >= 16384
    'small_600': (4, 0, 1, 1, 1),
    'small_1500': (8, 0, 1, 1, 1),
    'lattice_9000': (8, 0, 1, 3, 1),
    'pile': (8, 0, 1, 1, 1),
}
# sharded blocks (focal_begin, focal_count) and the forms of their LOCAL and REMOTE launches: (waves, resident, split)
BLOCKS = {
    'hall': ((2048, 1024), (8, 0, 1), (8, 0, 0)),             # both remote ranges non-empty
    'lattice_9000': ((4096, 1024), (8, 0, 1), (8, 0, 0)),     # remote range 0 is exactly one tile, range 1 spans a tile boundary
    'pile': ((1000, 500), (4, 0, 1), (4, 0, 0)),              # every source of range 0 ties at distance 0 with a lower index
}


@functools.lru_cache(maxsize=None)
def scene(name):
    build, kw = SCENES[name]
    sc = build(**kw)
    for x in sc.values():
        x.setflags(write=False)
    return sc


def geom(name, **over):
    return dict(GEOM.get(name, DEFAULT_GEOM), **over)


def dims(name):
    """(C, N, M) of a case"""
    sc = scene(name)
    p = sc['position']
    return (p.shape[0] if p.ndim == 3 else 1), p.shape[-2], sc['obstacles'].shape[0]


_REF = {}


def reference(oracle, name, **over):
    """oracle.relfeat_fwd of the case (with index and distance lists), computed once per geometry and left unchanged"""
    g = geom(name, **over)
    key = (name, tuple(sorted(g.items())))
    if key not in _REF:
        sc = scene(name)
        ref = oracle.relfeat_fwd(*[sc[k][..., None, :, :] for k in ('position', 'velocity', 'acceleration', 'destination')],
                                 sc['obstacles'], return_index=True, **g)
        for x in ref:
            x.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def plan(C, N, M, focal_count, topk_ped, topk_obs, part=0, has_pack=0):
    """piml_relfeat_plan -> (status, waves, resident, split, agent_tiles, obstacle_tiles); no GPU call is made"""
    from piml_amd import _lib
    out = [ctypes.c_int(-1) for _ in range(5)]
    r = _lib.lib().piml_relfeat_plan(C, N, M, focal_count, topk_ped, topk_obs, part, has_pack, *[ctypes.byref(x) for x in out])
    return (r,) + tuple(x.value for x in out)


def plan_of(name, part=0, focal_count=None, **over):
    C, N, M = dims(name)
    g = geom(name, **over)
    return plan(C, N, M, N if focal_count is None else focal_count, g['topk_ped'], g['topk_obs'], part)


# ---- what a scene contains, from the oracle's lists at topk = 32 (the tie group behind the cut is then in the list) ----
def cut_ties(idx, dist, k):
    """idx, dist: (rows, 32) lists in (distance, index) order.  -> (full rows, rows whose (k+1)-th entry ties with the k-th,
    the tie group's membership mask (rows, 32), zero outside those rows)"""
    idx, dist = idx.reshape(-1, idx.shape[-1]), dist.reshape(-1, dist.shape[-1])
    full = np.isfinite(dist[:, k - 1])
    tied = full & (dist[:, k] == dist[:, k - 1])
    group = (dist == dist[:, k - 1:k]) & tied[:, None] & (idx >= 0)
    return full, tied, group


def spans(idx, group, lo, mid, hi):
    """rows whose tie group holds a source in [lo, mid) and one in [mid, hi)"""
    idx = idx.reshape(-1, idx.shape[-1])
    return (group & (idx >= lo) & (idx < mid)).any(-1) & (group & (idx >= mid) & (idx < hi)).any(-1)


def within_cut(points, sources, kth_dist):
    """per row of `points`: how many of `sources` lie within the row's final k-th distance (exact: every coordinate is a multiple
    of 0.25, so the squared distance is exact and the float32 square root is the kernel's and the oracle's)"""
    out = np.zeros(len(points), np.int64)
    for r in np.nonzero(np.isfinite(kth_dist) & np.isfinite(points[:, 0]))[0]:
        d = sources - points[r]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32))
        out[r] = np.count_nonzero(dist <= kth_dist[r])
    return out
