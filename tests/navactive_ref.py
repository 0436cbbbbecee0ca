"""The weighted floor-field solve by active tiles (piml_nav_relax_active) restated in numpy float32 on navcost_ref.steps: two
buffers, a changed flag per 32 x 32 tile and launch, and the 3 x 3 dilation that decides which tiles the next launch steps.
A launch reads one buffer whole, takes 8 Jacobi steps, and writes ONLY its active tiles into the other buffer, so a tile the
scheme skips keeps whatever that buffer held: if skipping were not exact the field would differ from navcost_ref.solve's.
(The kernel steps a tile from a staged window with a halo of 8; for the tile's own cells that is the whole-grid step.)
reactivation_case() is a plan on which a tile goes quiet and wakes again; cases() the grids both test files run."""
import functools

import numpy as np

import nav_ref
import navcost_ref as COST

f32 = np.float32
TILE, STEPS = 32, 8


def tiles(gy, gx):
    return (gy + TILE - 1) // TILE, (gx + TILE - 1) // TILE


def dilate(flags):
    """flags (P, ty, tx) bool -> whether any of a tile's 3 x 3 neighbourhood is set; outside the tile grid counts as not"""
    P, ty, tx = flags.shape
    pad = np.zeros((P, ty + 2, tx + 2), bool)
    pad[:, 1:-1, 1:-1] = flags
    out = np.zeros_like(flags)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + ty, dx:dx + tx]
    return out


def plane_cost(cost, p, G):
    """plane p = member * G + gate reads cost[member] (cost (M, gy, gx)) or cost[member, gate] (cost (M, G, gy, gx))"""
    return cost[p // G] if cost.ndim == 3 else cost[p // G, p % G]


class Result:
    """u, other (M, G, gy, gx) float32: the buffer the last launch wrote and the one it read; active (launches, M G, ty, tx)
    bool; changed, the same shape: the flags each launch wrote; work (M, G) int64; launches; stalled"""


def relax_active(blocked, goal, cost, launches=None, limit=1 << 14):
    """launches = None: until a launch changed no tile (that launch counts); launches = n: exactly n.  The buffer launch 0
    reads holds the cold start, the other NaN: every word of it the result shows was written by a launch."""
    blocked, goal, cost = np.asarray(blocked), np.asarray(goal), np.asarray(cost, f32)
    G, gy, gx = goal.shape
    M = cost.shape[0]
    P, (ty, tx) = M * G, tiles(gy, gx)
    bufs = [np.tile(nav_ref.start(goal), (M, 1, 1, 1)).reshape(P, gy, gx).astype(f32), np.full((P, gy, gx), np.nan, f32)]
    flags = np.zeros((P, ty, tx), bool)
    active_maps, changed_maps = [], []
    n = 0
    while True:
        src, dst = bufs[n & 1], bufs[(n + 1) & 1]
        active = np.ones((P, ty, tx), bool) if n == 0 else dilate(flags)
        new = np.zeros((P, ty, tx), bool)
        for p in range(P):
            if not active[p].any():
                continue
            g = p % G
            nxt = COST.steps(src[p:p + 1], blocked, goal[g:g + 1], plane_cost(cost, p, G), STEPS)[0]
            for j, i in zip(*np.nonzero(active[p])):
                sl = (slice(j * TILE, (j + 1) * TILE), slice(i * TILE, (i + 1) * TILE))
                dst[p][sl] = nxt[sl]
                new[p, j, i] = not np.array_equal(nxt[sl].view(np.uint32), src[p][sl].view(np.uint32))
        active_maps.append(active)
        changed_maps.append(new)
        flags = new
        n += 1
        if (launches is None and not new.any()) or n == launches:
            break
        if n > limit:
            raise RuntimeError('no fixed point')
    r = Result()
    r.u, r.other = bufs[n & 1].reshape(M, G, gy, gx), bufs[(n + 1) & 1].reshape(M, G, gy, gx)
    r.active, r.changed = np.stack(active_maps), np.stack(changed_maps)
    r.work = r.active.sum((0, 2, 3)).reshape(M, G)
    r.launches, r.stalled = n, bool(flags.any())
    return r


def dense(blocked, goal, cost):
    """navcost_ref.solve of every plane: (u (M, G, gy, gx), the steps that changed something per plane (M, G))"""
    goal, cost = np.asarray(goal), np.asarray(cost, f32)
    G, M = goal.shape[0], cost.shape[0]
    u = np.empty((M, G) + goal.shape[1:], f32)
    steps = np.zeros((M, G), np.int64)
    for p in range(M * G):
        g = p % G
        v, steps[p // G, g] = COST.solve(blocked, goal[g:g + 1], plane_cost(cost, p, G))
        u[p // G, g] = v[0]
    return u, steps


# ---- the re-activation case ----
def reactivation_case():
    """161 x 65 (gx x gy): the border blocked; a wall on row 32 open at x = 1..3 and x = 150..152; the goal is cell (2, 16);
    the cost is 8 on rows 1..31, columns 6..145, and 1 elsewhere; the lower room holds a serpentine of walls every 4 columns
    from x = 8 to 144, even walls on rows 33..59 and odd ones on rows 37..63.  The first front reaches the upper room's far
    end slowly through the costly cells; the quick way round -- down the first door, through the serpentine, up the second
    -- arrives much later and lowers it again.  -> blocked (65, 161) uint8, goal (1, 65, 161) uint8, cost (65, 161) float32"""
    gx, gy = 161, 65
    blocked = np.zeros((gy, gx), np.uint8)
    blocked[0], blocked[-1], blocked[:, 0], blocked[:, -1] = 1, 1, 1, 1
    blocked[32] = 1
    blocked[32, 1:4] = 0
    blocked[32, 150:153] = 0
    for k, x in enumerate(range(8, 145, 4)):
        if k % 2 == 0:
            blocked[33:60, x] = 1
        else:
            blocked[37:64, x] = 1
    goal = np.zeros((1, gy, gx), np.uint8)
    goal[0, 16, 2] = 1
    cost = np.ones((gy, gx), f32)
    cost[1:32, 6:146] = 8
    return blocked, goal, cost


def histories(active):
    """active (launches, ty, tx) of ONE plane -> the tiles (j, i) that, after their first activity past launch 0, went
    quiet and were active again later"""
    out = []
    for j in range(active.shape[1]):
        for i in range(active.shape[2]):
            a = active[1:, j, i]
            on = np.nonzero(a)[0]
            if on.size and not a[on[0]:on[-1] + 1].all():
                out.append((j, i))
    return out


# ---- the cases of both test files: 3 members with different costs, 2 gates, both cost forms ----
GRIDS = ((1, 1), (40, 1), (33, 34), (65, 65))                # gx x gy


def _random_case(gx, gy):
    rng = np.random.default_rng(1000 * gx + gy)
    goal = np.zeros((2, gy, gx), np.uint8)
    goal[0, 0, 0] = 1
    goal[1, gy - 1, gx - 1] = 1
    blocked = (rng.random((gy, gx)) < 0.08).astype(np.uint8)
    blocked[:2, :2] = blocked[-2:, -2:] = 0                  # neither gate is walled in
    c3 = np.stack([np.ones((gy, gx)), 1 + 7 * rng.random((gy, gx)), rng.choice([1.0, 8.0], (gy, gx))]).astype(f32)
    c4 = np.stack([c3, (1 + 7 * rng.random((3, gy, gx))).astype(f32)], 1)
    return blocked, goal, c3, np.ascontiguousarray(c4, f32)


def _reactivation_planes():
    blocked, goal1, cost = reactivation_case()
    goal = np.zeros((2,) + goal1.shape[1:], np.uint8)
    goal[0] = goal1[0]
    goal[1, 48, 155] = 1                                     # a second gate, in the lower room past the serpentine
    c3 = np.stack([cost, np.ones_like(cost), np.where(cost > 1, f32(4), f32(1))]).astype(f32)
    c4 = np.ascontiguousarray(np.stack([c3, c3[[1, 2, 0]]], 1), f32)
    return blocked, goal, c3, c4


@functools.lru_cache(maxsize=None)
def case(name):
    """name: 'gx x gy' of GRIDS or 'reactivation' -> (blocked, goal (2, gy, gx), cost3 (3, gy, gx), cost4 (3, 2, gy, gx));
    the arrays are shared: leave them unchanged"""
    out = _reactivation_planes() if name == 'reactivation' else _random_case(*(int(n) for n in name.split('x')))
    for a in out:
        a.setflags(write=False)
    return out


CASES = tuple(f'{gx}x{gy}' for gx, gy in GRIDS) + ('reactivation',)


@functools.lru_cache(maxsize=None)
def solved(name, gates):
    """relax_active of case(name) with the cost per member (gates False) or per member and gate, computed once"""
    blocked, goal, c3, c4 = case(name)
    return relax_active(blocked, goal, c4 if gates else c3)
