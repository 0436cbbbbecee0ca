"""The inputs of test_metrics_edges_gpu.py and what test_metrics_edges.py checks of them without a GPU: frames for the
Sinkhorn OT and MMD kernels (piml_amd/csrc/metrics.hip) outside the region tests/golden/metrics_frames.npz covers -- masked
frames of more than one 1024-slot chunk, different masks (and slot counts) on the two sides, a handful of present points
among thousands of slots, eps and thresh other than 0.1.

Every set is (x (F, n, 2), mask_x (F, n), y (F, m, 2), mask_y (F, m)), float32, NaN in absent slots, built from SEEDS.  A
frame's present points are 20 * rand base points; x is a permuted subset of them, y another permuted subset plus
0.3 * randn (as the synthetic sets of golden/make_metrics_frames.py).  n >= m in every set.

  chunks   n = 2500, m = 1500 slots, 300 and 200 present, 4 frames whose masks are built (CHUNK_PATTERNS)
  sparse   2048 slots a side; present (x, y) = (3, 5), (2, 700), (1, 500), (500, 1), spread over both chunks
  small    n = 65, m = 64, every slot present: a wave's row loop runs a second round of one entry
  dense1k  n = 3000 with 1100 present, m = 2500 with 1000 present: 1024 threads masked and compacted alike
  perm     a 39 x 39 lattice of spacing 5 scattered in random slot order into n = 4000 slots, y the same points plus
           d = (0.3, -0.2) in another random order in m = 3000 slots (perm_relabelled: x in yet another slot order)

The float64 restatement of the reference's SinkhornDistance is sinkhorn64 of test_metrics_hip_gpu.py; sinkhorn32 here is
piml_amd.functions.metrics._sinkhorn_torch (the float32 restatement) line for line, returning the potentials as well and
taking thresh (test_metrics_edges.py asserts the two give the same bits at thresh 0.1)."""
import functools
import os
import re

import numpy as np
import torch

from test_metrics_hip_gpu import in_band, sinkhorn64

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'piml_amd', 'csrc')
CHUNK = 1024                                  # what the tests below call a chunk; == thread_limits()[1] (asserted on the CPU)
WAVE = 64
EPS = (0.01, 0.1, 1.0)                        # with the reference's thresh, 0.1
EXTRA = ((0.1, 1e-3), (0.05, 0.01))           # (eps, thresh): float64 restatement only, the reference's thresh is fixed
REF_THRESH = 0.1
SEEDS = dict(chunks=101, sparse=102, small=103, dense1k=104, perm=105, functions=106)
SPARSE_COUNTS = ((3, 5), (2, 700), (1, 500), (500, 1))
PERM_SIDE, PERM_STEP, PERM_D = 39, 5.0, (0.3, -0.2)
GROUPS = tuple((s, e, REF_THRESH) for s in ('chunks', 'sparse', 'small') for e in EPS) + \
    tuple((s, e, t) for s in ('chunks', 'sparse', 'small') for e, t in EXTRA)      # sparse: stops early, so thresh decides


def thread_limits():
    """(floor, cap) of metric_threads in metrics.hip, read out of its source"""
    with open(os.path.join(CSRC, 'metrics.hip')) as fh:
        text = fh.read()
    body = re.findall(r'static int metric_threads\(int n, int m\)\s*\{(.*?)\n\}', text, re.S)
    if len(body) != 1:
        raise ValueError(f'metric_threads: {len(body)} definitions in metrics.hip')
    found = re.findall(r'return t < (\d+) \? (\d+) : \(t > (\d+) \? (\d+) : t\);', body[0])
    if len(found) != 1 or found[0][0] != found[0][1] or found[0][2] != found[0][3] or '(p + 63) / 64 * 64' not in body[0]:
        raise ValueError('metric_threads: its body is not the one restated here')
    return int(found[0][0]), int(found[0][2])


def metric_threads(n, m):
    """the workgroup size of a call with n and m slots (metric_threads restated)"""
    lo, hi = thread_limits()
    return min(max((max(n, m) + 63) // 64 * 64, lo), hi)


# ----------------------------------------------------------------------------------------------------------------------
# frames
def _cloud(g, cx, cy):
    base = 20 * torch.rand(max(cx, cy), 2, generator=g)
    x = base[torch.randperm(base.shape[0], generator=g)[:cx]]
    y = base[torch.randperm(base.shape[0], generator=g)[:cy]]
    return x, y + 0.3 * torch.randn(cy, 2, generator=g)


def _slots(g, count, allowed, forced=()):
    """`count` sorted slots: the forced ones and random picks among the allowed ones"""
    forced = sorted(set(int(s) for s in forced))
    rest = np.setdiff1d(np.asarray(list(allowed), dtype=np.int64), forced)
    pick = rest[torch.randperm(len(rest), generator=g)[:count - len(forced)].numpy()]
    out = np.sort(np.concatenate((np.asarray(forced, dtype=np.int64), pick)))
    assert len(out) == count, (len(out), count)
    return torch.from_numpy(out)


def _scatter(points, slots, n):
    """points[k] at slot slots[k] of an n-slot frame, NaN elsewhere -> (n, 2), mask (n)"""
    frame = torch.full((n, 2), float('nan'))
    mask = torch.zeros(n)
    frame[slots] = points
    mask[slots] = 1
    return frame, mask


def _stack(frames):
    x, mx, y, my = zip(*frames)
    return torch.stack(x), torch.stack(mx), torch.stack(y), torch.stack(my)


def _span(*ranges):
    return [s for a, b in ranges for s in range(a, b)]


def CHUNK_PATTERNS(n, m):
    """per frame of `chunks`: (x allowed, x forced, y allowed, y forced)"""
    C, W = CHUNK, WAVE
    return (
        # present slots on both sides of every chunk boundary, and the last slot
        (range(n), (C - 1, C, 2 * C - 1, 2 * C, n - 1), range(m), (C - 1, C, m - 1)),
        # x: chunk 1 holds nothing; y: chunk 0 holds nothing
        (_span((0, C), (2 * C, n)), (), range(C, m), ()),
        # a whole wave present next to one wholly absent, in chunk 0 and in chunk 1 of x and in chunk 1 of y
        (_span((0, 2 * W), (3 * W, C + 4 * W), (C + 5 * W, n)), _span((W, 2 * W), (C + 3 * W, C + 4 * W)),
         _span((0, C + W), (C + 2 * W, m)), _span((C, C + W))),
        # x: chunk 0 holds nothing, so the first present point lies in chunk 1
        (range(C, n), (n - 1,), range(m), (0, C - 1, C)),
    )


@functools.lru_cache(maxsize=None)
def frames(name):
    g = torch.Generator().manual_seed(SEEDS[name.split('_')[0]])
    if name == 'chunks':
        n, m, cx, cy = 2500, 1500, 300, 200
        out = []
        for ax, fx, ay, fy in CHUNK_PATTERNS(n, m):
            x, y = _cloud(g, cx, cy)
            out.append(_scatter(x, _slots(g, cx, ax, fx), n) + _scatter(y, _slots(g, cy, ay, fy), m))
        return _stack(out)
    if name == 'sparse':
        n = 2 * CHUNK
        out = []
        for f, (cx, cy) in enumerate(SPARSE_COUNTS):
            x, y = _cloud(g, cx, cy)
            sides = []
            for c, lone in ((cx, CHUNK + 476 + f), (cy, 700 + f)):      # a lone point: x's in chunk 1, y's in chunk 0
                forced = (lone,) if c == 1 else (int(torch.randint(0, CHUNK, (1,), generator=g)),
                                                 CHUNK + int(torch.randint(0, CHUNK, (1,), generator=g)))
                sides.append(_slots(g, c, range(n), forced))
            out.append(_scatter(x, sides[0], n) + _scatter(y, sides[1], n))
        return _stack(out)
    if name == 'small':
        out = []
        for _ in range(3):
            x, y = _cloud(g, 65, 64)
            out.append(_scatter(x, torch.arange(65), 65) + _scatter(y, torch.arange(64), 64))
        return _stack(out)
    if name == 'dense1k':
        out = []
        for _ in range(2):
            x, y = _cloud(g, 1100, 1000)
            out.append(_scatter(x, _slots(g, 1100, range(3000)), 3000) + _scatter(y, _slots(g, 1000, range(2500)), 2500))
        return _stack(out)
    if name in ('perm', 'perm_relabelled'):
        k = torch.arange(PERM_SIDE, dtype=torch.float32) * PERM_STEP
        lattice = torch.stack(torch.meshgrid(k, k, indexing='ij'), -1).reshape(-1, 2)
        sx, sy, sx2 = (torch.randperm(s, generator=g)[:lattice.shape[0]] for s in (4000, 3000, 4000))
        return _stack([_scatter(lattice, sx2 if name == 'perm_relabelled' else sx, 4000)
                       + _scatter(lattice + torch.tensor(PERM_D), sy, 3000)])
    raise KeyError(name)


def compacted(name, f):
    """frame f's present points in slot order, as the reference's p[mask == 1]: x (cx, 2), y (cy, 2)"""
    x, mx, y, my = frames(name)
    return x[f][mx[f] == 1], y[f][my[f] == 1]


def n_frames(name):
    return frames(name)[0].shape[0]


@functools.lru_cache(maxsize=None)
def functions_input():
    """p, q (T, 2500, 2) and mask (T, 2500) for the functions layer: the x side of `chunks` and a perturbed copy"""
    p, mask, _, _ = frames('chunks')
    g = torch.Generator().manual_seed(SEEDS['functions'])
    return p, p + 0.3 * torch.randn(p.shape, generator=g), mask


@functools.lru_cache(maxsize=None)
def degenerate():
    """`sparse` with a degenerate frame after each of its own: x empty, y empty, both empty, one point a side.  Returns
    (x, mask_x, y, mask_y, keep) with keep the positions of sparse's frames."""
    x, mx, y, my = (t.clone() for t in frames('sparse'))
    nan = float('nan')
    dx, dmx, dy, dmy = x.clone(), mx.clone(), y.clone(), my.clone()
    dx[0], dmx[0] = nan, 0                                                # x empty, y as sparse frame 0 (5 points)
    dy[1], dmy[1] = nan, 0                                                # y empty, x as sparse frame 1 (2 points)
    dx[2], dmx[2], dy[2], dmy[2] = nan, 0, nan, 0                         # both empty
    dx[3], dmx[3] = dx[2], dmx[2]                                         # one point a side: x at slot 1500, y as frame 3
    dx[3, 1500], dmx[3, 1500] = torch.tensor([3.0, 4.5]), 1
    order = [0, 4, 1, 5, 2, 6, 3, 7]
    cat = [torch.cat((a, b))[order] for a, b in ((x, dx), (mx, dmx), (y, dy), (my, dmy))]
    return (*cat, [0, 2, 4, 6])


# ----------------------------------------------------------------------------------------------------------------------
# restatements
def sinkhorn32(x, y, eps=0.1, max_iter=100, thresh=REF_THRESH):
    """_sinkhorn_torch (piml_amd/functions/metrics.py) on one float32 frame, with thresh an argument: (cost, iterations,
    u, v)"""
    from piml_amd.functions.metrics import _cost_matrix
    x, y = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(y, dtype=torch.float32)
    C = _cost_matrix(x, y)
    log_mu = torch.log(torch.full((x.shape[-2],), 1.0 / x.shape[-2], dtype=torch.float32) + 1e-8)
    log_nu = torch.log(torch.full((y.shape[-2],), 1.0 / y.shape[-2], dtype=torch.float32) + 1e-8)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)

    def M(u_, v_):
        return (-C + u_.unsqueeze(-1) + v_.unsqueeze(-2)) / eps
    it = 0
    for _ in range(max_iter):
        u_prev = u
        u = eps * (log_mu - torch.logsumexp(M(u, v), dim=-1)) + u
        v = eps * (log_nu - torch.logsumexp(M(u, v).transpose(-2, -1), dim=-1)) + v
        it += 1
        if (u - u_prev).abs().sum(-1).mean().item() < thresh:
            break
    return float((torch.exp(M(u, v)) * C).sum(dim=(-2, -1))), it, u, v


@functools.lru_cache(maxsize=None)
def ref64(name, eps, thresh=REF_THRESH, max_iter=100):
    """sinkhorn64 of every frame of a set: a list of (cost, iterations, errs, u, v)"""
    return [sinkhorn64(*compacted(name, f), eps=eps, max_iter=max_iter, thresh=thresh, potentials=True)
            for f in range(n_frames(name))]


@functools.lru_cache(maxsize=None)
def ref32(name, eps, thresh=REF_THRESH, max_iter=100):
    """sinkhorn32 of every frame of a set: a list of (cost, iterations, u, v)"""
    return [sinkhorn32(*compacted(name, f), eps=eps, max_iter=max_iter, thresh=thresh) for f in range(n_frames(name))]


def band_frames(name, eps, thresh=REF_THRESH):
    """the frames of a set whose float64 err passes within BAND of thresh where it stops: float32 may stop one apart"""
    return [f for f, r in enumerate(ref64(name, eps, thresh)) if in_band(r[2], thresh)]


def cost_tolerance(g, name, eps):
    """the relative bound on a (set, eps) group's costs against the reference's recorded float32 values: 3 x the largest
    relative distance in the group between the reference on float32 and on float64 inputs, 1e-5 at the least (a frame
    the reference cannot run, recorded as NaN, has no spread)"""
    r32, r64 = g[f'{name}/ot32_{eps}'], g[f'{name}/ot64_{eps}']
    return max(1e-5, 3 * float(np.nanmax(np.abs(r32 - r64) / np.abs(r64))))


def restated_cost_tolerance(name, eps, thresh):
    """the same bound for an (eps, thresh) the reference cannot run, from the float32 and float64 restatements"""
    spread = [abs(a[0] - b[0]) / abs(b[0]) for a, b in zip(ref32(name, eps, thresh), ref64(name, eps, thresh))]
    return max(1e-5, 3 * max(spread))


def potential_tolerance(name, eps=0.1):
    """the absolute bound on a group's potentials against float64: 3 x the float32 restatement's largest |u32 - u64|; and
    the restatement's largest |v32 - v64| for the record"""
    du = max(float((a[2].double() - b[3]).abs().max()) for a, b in zip(ref32(name, eps), ref64(name, eps)))
    dv = max(float((a[3].double() - b[4]).abs().max()) for a, b in zip(ref32(name, eps), ref64(name, eps)))
    return 3 * du, dv


def one_against_many(x, y):
    """the forced plan's cost, float64.  One x point: the v half-step makes every column's mass 1/m + 1e-8.  One y point:
    the u half-step gives the rows equal mass and the v half-step scales their sum to 1 + 1e-8."""
    x, y = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64)
    C = ((x.unsqueeze(-2) - y.unsqueeze(-3)) ** 2).sum(-1)
    if x.shape[0] == 1:
        return float(((1.0 / y.shape[0] + 1e-8) * C).sum())
    assert y.shape[0] == 1
    return float(((1.0 + 1e-8) / x.shape[0] * C).sum())


def perm_cost():
    """the matching's cost: every pair at |d|^2 with mass 1/1521 + 1e-8"""
    k = PERM_SIDE * PERM_SIDE
    d2 = float(np.float64(np.float32(PERM_D[0])) ** 2 + np.float64(np.float32(PERM_D[1])) ** 2)
    return d2 * (1 + k * 1e-8)
