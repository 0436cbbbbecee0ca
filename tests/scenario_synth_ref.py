"""numpy restatement of the scene rules of the open-world frame (piml_scenario_step_rules, piml_amd/csrc/scenario.hip)
for the tests: the Philox word layout of the synthetic scenes' spawn laws (stream c3 = 0x5CE10000 | sub), the square's
randperm, and the integrate / arrive / retire rule of one frame.

  counts of frame f        philox(f lo, f hi, 0, 0x5CE10000): k1 = #{j < cap : w0 >> 8 >= thr[j]}, k2 likewise from w1
  agent n, call 1          philox(n lo, n hi, 0, 0x5CE10001): the law's coins (w >> 31) and uniforms ((w >> 8) 2^-24)
  agent n, call 2          philox(n lo, n hi, 0, 0x5CE10002): z = sqrt(-2 ln u1) cos(2 pi u2) (double), as GC's call 3
  square cell c            philox(c, 0, 0, 0x5CE10003) word 0: randperm[c] = its rank among the d^2 keys, ties by index
"""
import numpy as np

from philox_ref import philox4x32_10
from scenario_ref import _norm

STREAM = 0x5CE10000
f32 = np.float32
U24 = f32(2.0 ** -24)


def _words(seed, idx, sub):
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & np.uint64(0xffffffff), idx >> np.uint64(32)
    zero = np.zeros_like(idx)
    return philox4x32_10(lo, hi, zero, zero + np.uint64(STREAM | sub), seed & 0xffffffff, (seed >> 32) & 0xffffffff)


def _u(w):
    return (w >> np.uint32(8)).astype(np.float32) * U24


def _coin(w):
    return (w >> np.uint32(31)).astype(bool)


def spawn_counts(seed, frames, thr1, thr2):
    """(k1, k2) of each frame index in `frames`."""
    w = _words(seed, frames, 0)
    c = lambda x, t: (x.astype(np.uint64)[:, None] >= np.asarray(t, np.uint64)[None, :]).sum(1).astype(np.int64)
    return c(w[0] >> np.uint32(8), thr1), c(w[1] >> np.uint32(8), thr2)


def schedule(seed, frames, n_initial, thr1, thr2):
    """(frame of each ordinal, stream (0 / 1) of each ordinal, per-frame counts (frames,)) of a free-running simulation."""
    k1, k2 = spawn_counts(seed, np.arange(1, frames), thr1, thr2)
    counts = np.concatenate(([n_initial], k1 + k2))
    born = np.repeat(np.arange(frames), counts)
    group = np.concatenate([np.zeros(n_initial, np.int64)] +
                           [np.repeat([0, 1], [a, b]) for a, b in zip(k1, k2)]).astype(np.int64)
    return born, group, counts


def square_perm(seed, d):
    key = _words(seed, np.arange(d * d), 3)[0].astype(np.int64)
    order = np.lexsort((np.arange(d * d), key))          # by key, ties by index
    rank = np.empty(d * d, np.int64)
    rank[order] = np.arange(d * d)
    return rank


def speeds(sc, seed, ordinals):
    n = len(ordinals)
    if sc.uniform_desired_speed:
        return np.full(n, sc.speed_mean, np.float32)
    w = _words(seed, ordinals, 2)
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    z = (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(np.float32)
    v0 = f32(sc.speed_mean) + f32(sc.speed_var ** 0.5) * z
    if sc.speed_clamp:
        v0 = np.where(v0 < f32(sc.speed_min), f32(sc.speed_min), v0)
    return v0.astype(np.float32)


def spawn(sc, seed, ordinals, group=None):
    """position, velocity (n, 2), waypoints (D, n, 2), desired speed (n) of the agents `ordinals` (stream `group`)."""
    ordinals = np.asarray(ordinals, np.int64)
    n = len(ordinals)
    group = np.zeros(n, np.int64) if group is None else np.asarray(group)
    L, W = f32(sc.length), f32(sc.width)
    half_L, half_W = f32(0.5) * L, f32(0.5) * W
    wp1 = np.full((n, 2), np.nan, np.float32)
    head = np.zeros((n, 2), np.float32)
    jit = lambda w: f32(2) * _u(w) - f32(1)
    law = sc.spawn_law
    if law == 'square':
        g = sc.square_grid.numpy()
        d = len(g)
        c, blk = ordinals % (d * d), ordinals // (d * d)
        s = square_perm(seed, d)[c]
        gx, gy, hx, hy = g[c // d], g[c % d], g[s // d], g[s % d]
        ox = np.select([blk == 0, blk == 1], [gx - L, gx + L], gx)
        oy = np.select([blk == 2, blk == 3], [gy - L, gy + L], gy)
        dx = np.select([blk == 0, blk == 1], [hx + L, hx - L], hx)
        dy = np.select([blk == 2, blk == 3], [hy + L, hy - L], hy)
    else:
        w = _words(seed, ordinals, 1)
        if law == 'crosswalk':
            sx = np.where(_coin(w[0]), f32(1), f32(-1))
            sy = np.where(_coin(w[1]), f32(1), f32(-1))
            ox = sx * (half_L + f32(3) * _u(w[2]))
            oy = half_W * sy
            dx = -sx * half_L
            dy = -half_W + np.where(_coin(w[3]), W, f32(0))
            wp1 = np.stack((dx, dy * f32(3)), -1)
            head[:, 1] = -sy
        elif law == 'unit2':
            left, rtl = _u(w[0]) < f32(sc.side_ratio), _u(w[1]) < f32(sc.direction_ratio)
            y = half_W * _u(w[2])
            y = np.where(left, y + half_W, y)
            y = np.where(rtl, W - y, y)
            ox, oy = np.where(rtl, L, f32(0)), y
            dx, dy = np.where(rtl, f32(0), L), y + jit(w[3])
            head[:, 0] = np.where(rtl, -1, 1)
        else:                                            # unit1, unit3 (stream 1 / stream 2)
            g2 = (group == 1) if law == 'unit3' else np.zeros(n, bool)
            y = W * _u(w[0])
            x = L * _u(w[0])
            ox, oy = np.where(g2, x, f32(0)), np.where(g2, f32(0), y)
            dx, dy = np.where(g2, x + jit(w[1]), L), np.where(g2, W, y + jit(w[1]))
            head[:, 0], head[:, 1] = ~g2, g2
    v0 = speeds(sc, seed, ordinals)
    vel = np.where(head != 0, head * v0[:, None], f32(0)) if sc.initial_velocity else np.zeros((n, 2), np.float32)
    D = sc.num_waypoints
    wp = np.full((D, n, 2), np.nan, np.float32)
    wp[0] = np.stack((dx, dy), -1)
    if D > 1:
        wp[1] = wp1
    return np.stack((ox, oy), -1).astype(np.float32), vel.astype(np.float32), wp, v0


def step(sc, state, a_next, dt):
    """Integrate / arrive / retire of the present agents of `state` (dict: p, v, a, dest, flag, mask, waypoints);
    returns the new dict (spawning not included)."""
    s = {k: np.array(v) for k, v in state.items()}
    live = s['mask'] == 1
    dtf = f32(dt)
    vn = (s['v'] + s['a'] * dtf).astype(np.float32)
    pn = (s['p'] + s['v'] * dtf).astype(np.float32)
    d = s['dest']
    flag = s['flag'].copy()
    gone = np.zeros_like(live)
    with np.errstate(invalid='ignore'):
        if sc.arrival_rule == 'radius':
            flag += live & (_norm(pn[:, 0] - d[:, 0], pn[:, 1] - d[:, 1]) < f32(sc.arrival_radius))
        elif sc.arrival_rule == 'x_band':
            flag += live & (np.abs(pn[:, 0] - d[:, 0]) < f32(sc.arrival_radius))
        else:
            gone = live & (pn[:, 0] > f32(sc.length))
    D = s['waypoints'].shape[0]
    newdest = np.full_like(d, np.nan)
    for i in np.nonzero(live)[0]:
        if gone[i] or flag[i] >= D or np.isnan(s['waypoints'][flag[i], i]).any():
            gone[i] = True
        else:
            newdest[i] = s['waypoints'][flag[i], i]
    keep = live & ~gone
    nan = np.float32(np.nan)
    out = dict(s)
    out['p'] = np.where(keep[:, None], pn, np.where(live[:, None], nan, s['p'])).astype(np.float32)
    out['v'] = np.where(keep[:, None], vn, np.where(live[:, None], 0, s['v'])).astype(np.float32)
    out['a'] = np.where(keep[:, None], a_next, np.where(live[:, None], 0, s['a'])).astype(np.float32)
    out['dest'] = np.where(live[:, None], newdest, d).astype(np.float32)
    out['flag'] = np.where(live, flag, s['flag'])
    out['mask'] = np.where(gone, 0, s['mask']).astype(np.float32)
    return out
