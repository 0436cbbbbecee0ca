"""Scene builders and a plain reference for the collision predicates (numpy only).

The collision counts are integers, so every comparison built on this module is exact.  Three kinds of scene:

near_threshold_scene    designated pairs whose float32 distance lies within a few ulp of the threshold, on both sides and
                        exactly on it: the only pairs for which a squared-domain cut that is one float off, or the naive
                        thr * thr, changes a count;
friends_boundary_scene  designated pairs that collide in exactly 24, 25, 26 and 27 slices (the friends rule keeps a pair up
                        to 25 and drops it from 26), one pair whose totals differ between the two thresholds, one that
                        reaches 25 only because an agent is absent in some slices, one that collides in every slice;
lattice_scene           positions on a 0.25 m lattice: at the thresholds 0.25, 0.5 and 1.0 every arithmetic (float32,
                        float64, squared or not) gives the same predicate, so counts_ref below is exact for it at any size.
"""
import functools

import numpy as np

F32 = np.float32


def d2_f32(a, b):
    """Squared distance as the oracle and the kernels evaluate it: fmaf(ry, ry, rx * rx) on float32 differences (the
    product ry * ry is exact in float64; the second rounding of the sum through float64 can differ from a true fma only
    on a float64 tie, about one case in 2^29)."""
    rx = (b[..., 0] - a[..., 0]).astype(F32)
    ry = (b[..., 1] - a[..., 1]).astype(F32)
    xx = (rx * rx).astype(F32)
    return (ry.astype(np.float64) * ry.astype(np.float64) + xx.astype(np.float64)).astype(F32)


def dist_f32(a, b):
    return np.sqrt(d2_f32(a, b), dtype=F32)


@functools.lru_cache(maxsize=None)
def near_threshold_scene(thr, npairs, S, seed):
    """(S, 2 * npairs, 2) float32, pair m = agents (2 m, 2 m + 1).  Anchors on a grid spaced 4 thr with jitter in
    [0, thr); the partner aims at the distance thr (1 + k 2^-24), k in -4 .. 4, and takes, of the slice's 2048 random
    directions, the one whose float32 distance (after rounding the partner's position) comes closest to that.  Every slice is
    drawn on its own.  The array is cached: do not write to it."""
    rng = np.random.default_rng(seed)
    t = float(F32(thr))
    side = int(np.ceil(np.sqrt(npairs)))
    m = np.arange(npairs)
    grid = np.stack([m % side, m // side], -1) * (4.0 * t)
    out = np.empty((S, 2 * npairs, 2), F32)
    rows = np.arange(npairs)
    for s in range(S):
        a = (grid + rng.random((npairs, 2)) * t).astype(F32)
        k = rng.integers(-4, 5, size=npairs)
        target = t * (1.0 + k * 2.0 ** -24)
        ang = rng.random(2048) * (2 * np.pi)                           # one set of directions a slice
        step = target[:, None, None] * np.stack([np.cos(ang), np.sin(ang)], -1)[None]
        b = (a[:, None, :].astype(np.float64) + step).astype(F32)
        err = np.abs(dist_f32(a[:, None, :], b).astype(np.float64) - target[:, None])
        best = err.argmin(1)
        out[s, 0::2] = a
        out[s, 1::2] = b[rows, best]
    out.setflags(write=False)
    return out


def sq_cut(thr):
    """Largest float32 y with sqrt(y) < thr (float32, correctly rounded), found by search from thr * thr: the cut of
    "sqrtf(d2) < thr  <=>  d2 <= y".  thr > 0."""
    t = F32(thr)
    y = F32(t * t)
    while np.sqrt(y, dtype=F32) >= t:
        y = np.nextafter(y, F32(-np.inf))
    while np.sqrt(np.nextafter(y, F32(np.inf)), dtype=F32) < t:
        y = np.nextafter(y, F32(np.inf))
    return y


def friends_boundary_scene(S, thr_pair, seed, nbg=90):
    """(p, pairs): p (S, N, 2) float32 and pairs = {name: (i, j, total at thr_hi, total at thr_lo)}, the number of slices
    in which the designated pair (i, j) collides.  thr_pair = (thr_hi, thr_lo) with 0.1 < thr_lo < 0.6 thr_hi.

    Background agents sit 4 thr_hi apart with a jitter below thr_hi (5 % absent): they never collide.  A designated pair
    is 0.1 m apart in its colliding slices and 3 thr_hi apart in the others.  A pair that collides in n slices does so in
    slices 0 .. n - 2 and in the last one, so that with more than 32 slices its total is built from two chunks.
      c24, c25, c26, c27   n = 24 .. 27 (left out, total 0, where n > S)
      split                0.1 m apart in 25 slices and 0.6 thr_hi apart in one more: 26 at thr_hi, 25 at thr_lo
      absent               at the same point in the first min(30, S) slices, one agent absent in all but 25 of them
      always               colliding in every slice
    The agents are shuffled, so the pairs are spread over the index range."""
    hi, lo = float(thr_pair[0]), float(thr_pair[1])
    assert 0.1 < lo < 0.6 * hi
    rng = np.random.default_rng(seed)
    names = ['c24', 'c25', 'c26', 'c27', 'split', 'absent', 'always']
    N = nbg + 2 * len(names)
    p = np.empty((S, N, 2), F32)
    side = int(np.ceil(np.sqrt(nbg)))
    m = np.arange(nbg)
    p[:, :nbg] = np.stack([m % side, m // side], -1) * (4.0 * hi) + rng.random((S, nbg, 2)) * (0.9 * hi)
    p[:, :nbg][rng.random((S, nbg)) < 0.05] = np.nan
    near, far = np.array([0.1, 0.0]), np.array([3.0 * hi, 0.0])
    totals = {}
    for q, name in enumerate(names):
        a = np.array([-20.0 * hi, 8.0 * hi * q])                       # a column of anchors left of the background
        i, j = nbg + 2 * q, nbg + 2 * q + 1
        p[:, i] = a
        p[:, j] = a + far
        if name.startswith('c'):
            n = int(name[1:])
            if n <= S:
                sl = list(range(n - 1)) + [S - 1]
                p[sl, j] = a + near
                totals[name] = (n, n)
            else:
                totals[name] = (0, 0)
        elif name == 'split':
            nn = min(24, S - 2)                                        # 26 and 25 from 26 slices on
            p[list(range(nn)) + [S - 1], j] = a + near
            p[nn, j] = a + np.array([0.0, 0.6 * hi])
            totals[name] = (nn + 2, nn + 1)
        elif name == 'absent':
            n = min(30, S)
            p[:n, j] = a
            p[25:n, i] = np.nan
            totals[name] = (25, 25)
        else:
            p[:, j] = a + near
            totals[name] = (S, S)
    perm = rng.permutation(N)
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    p = np.ascontiguousarray(p[:, perm])
    pairs = {name: (int(inv[nbg + 2 * q]), int(inv[nbg + 2 * q + 1])) + totals[name] for q, name in enumerate(names)}
    return p, pairs


def lattice_scene(S, N, extent, seed, nan_frac=0.05):
    """(S, N, 2) float32 on the 0.25 m lattice over [-extent, extent): a base position per agent plus a step of -1, 0
    or 1 lattice units per slice and axis (so pairs stay together over many slices), a fraction nan_frac absent."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-4 * extent, 4 * extent, size=(1, N, 2))
    p = ((base + rng.integers(-1, 2, size=(S, N, 2))) * 0.25).astype(F32)
    p[rng.random((S, N)) < nan_frac] = np.nan
    return p


def counts_ref(p, thr):
    """collision_detection(p (S, N, 2), thr).sum(-1) with the 3-D friends rule, in float64, one slice at a time and
    without any (S, N, N) array: the colliding ordered pairs of each slice as a list, a pair's total = the number of
    slices that list it, a pair with a total above 25 dropped everywhere.  Exact for lattice scenes (see the module's
    head); absent agents collide with nobody.  Within a slice the agents are sorted by x, and a block of rows is tested
    against the agents within thr of its x range only (everybody else is at least thr away)."""
    p = np.asarray(p, np.float64)
    S, N = p.shape[0], p.shape[1]
    thr = float(F32(thr))
    keys = []
    for s in range(S):
        idx = np.nonzero(~np.isnan(p[s]).any(-1))[0]
        idx = idx[np.argsort(p[s, idx, 0], kind='stable')]
        x, y = p[s, idx, 0], p[s, idx, 1]
        found = []
        for r0 in range(0, len(idx), 256):
            r1 = min(len(idx), r0 + 256)
            c0 = np.searchsorted(x, x[r0] - thr, 'left')
            c1 = np.searchsorted(x, x[r1 - 1] + thr, 'right')
            dx = x[None, c0:c1] - x[r0:r1, None]
            dy = y[None, c0:c1] - y[r0:r1, None]
            hit = np.sqrt(dx * dx + dy * dy) < thr
            ri, ci = np.nonzero(hit)
            i, j = idx[r0 + ri], idx[c0 + ci]
            keep = i != j
            found.append(i[keep] * N + j[keep])
        keys.append(np.concatenate(found) if found else np.empty(0, np.int64))
    every = np.concatenate(keys) if keys else np.empty(0, np.int64)
    pair, total = np.unique(every, return_counts=True)
    friends = pair[total > 25]
    counts = np.zeros((S, N), F32)
    for s in range(S):
        k = keys[s][~np.isin(keys[s], friends)]
        counts[s] = np.bincount(k // N, minlength=N)
    return counts
