"""numpy restatement of the open-world scenario frame (piml_amd/csrc/scenario.hip) for the tests, in the style of
philox_ref.py: the Philox word layout of the spawn stream, utils.route (src/utils/utils.py:141-165) in float32, and the
integrate / arrive / retire rule of one frame.

Spawn stream (key = (seed lo, seed hi)):
  count of frame f       philox(f lo, f hi, 0, 0x5CE00000) word 0 >> 8 = u24; k = #{j < spawn_cap : u24 >= thr[j]}
  agent n, call 1        philox(n lo, n hi, 0, 0x5CE00001): origin entry (w0 E) >> 32, destination entry (w1 (E-1)) >> 32
                         shifted past the origin, origin point (w2 P) >> 32, destination point (w3 P) >> 32
  agent n, call 2        philox(n lo, n hi, 0, 0x5CE00002): offsets (w >> 8) 2^-24: origin (w0, w1), destination (w2, w3)
  agent n, call 3        philox(n lo, n hi, 0, 0x5CE00003): z = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((w0 >> 8) + 1) 2^-24,
                         u2 = (w1 >> 8) 2^-24 (double)
"""
import numpy as np

from philox_ref import philox4x32_10

STREAM = 0x5CE00000
U24 = np.float32(2.0 ** -24)
f32 = np.float32


def _key(seed):
    return seed & 0xffffffff, (seed >> 32) & 0xffffffff


def _words(seed, idx, sub):
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & np.uint64(0xffffffff), idx >> np.uint64(32)
    zero = np.zeros_like(idx)
    return philox4x32_10(lo, hi, zero, zero + np.uint64(STREAM | sub), *_key(seed))


def spawn_counts(seed, frames, thresholds):
    """k of each frame index in `frames` (int array)."""
    u = _words(seed, frames, 0)[0] >> np.uint32(8)
    thr = np.asarray(thresholds, dtype=np.uint64)
    return (u.astype(np.uint64)[:, None] >= thr[None, :]).sum(1).astype(np.int64)


def _pick(w, n):
    return ((w.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def agent_draws(seed, ordinals, E, P):
    """dict of the integer choices, offsets (float32) and standard normal z (float32) of each ordinal."""
    w1, w2, w3 = (_words(seed, ordinals, s) for s in (1, 2, 3))
    oe = _pick(w1[0], E)
    de = _pick(w1[1], E - 1)
    de = de + (de >= oe)
    u = [(x >> np.uint32(8)).astype(np.float32) * U24 for x in w2]
    u1 = ((w3[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w3[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    z = (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(np.float32)
    return dict(oe=oe, de=de, oi=_pick(w1[2], P), di=_pick(w1[3], P), uo=np.stack(u[:2], -1), ud=np.stack(u[2:], -1), z=z)


def spawn_agents(seed, ordinals, entries, spawn_offset=0.8, speed_mean=1.34, speed_var=0.26, speed_min=0.7, uniform=False):
    """origin o, destination d (n, 2) float32, desired speed (n) float32, and the draws."""
    E, P = entries.shape[0], entries.shape[1]
    dr = agent_draws(seed, ordinals, E, P)
    off = f32(spawn_offset)
    o = entries[dr['oe'], dr['oi']] + dr['uo'] * off
    d = entries[dr['de'], dr['di']] + dr['ud'] * off
    if uniform:
        v0 = np.full(len(o), speed_mean, np.float32)
    else:
        v0 = f32(speed_mean) + f32(speed_var ** 0.5) * dr['z']
        v0 = np.where(v0 < f32(speed_min), f32(speed_min), v0).astype(np.float32)
    return o.astype(np.float32), d.astype(np.float32), v0, dr


def schedule(seed, frames, n_initial, thresholds, capacity=None):
    """(frame of each ordinal (int64), per-frame counts (frames,)) of a free-running simulation of `frames` frames."""
    k = spawn_counts(seed, np.arange(1, frames), thresholds)
    counts = np.concatenate(([n_initial], k))
    born = np.repeat(np.arange(frames), counts)
    return born, counts


def _norm(x, y):
    """torch.norm's float32 arithmetic on a 2-vector: sqrt(fma(y, y, x * x))."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    y64 = np.asarray(y, np.float32).astype(np.float64)
    return np.sqrt((y64 * y64 + (x64 * x64).astype(np.float32).astype(np.float64)).astype(np.float32))


def route(o, d, poly, max_iters=16, clearance=2.0):
    """utils.route for every pair: (r (n, 2) float32, iters (n))."""
    o = np.asarray(o, np.float32)
    r = np.array(d, np.float32)
    poly = np.asarray(poly, np.float32)
    B = poly[1:] - poly[:-1]
    iters = np.zeros(len(o), np.int64)
    live = np.ones(len(o), bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for _ in range(max_iters):
            A = r - o
            C = poly[None, :-1, :] - o[:, None, :]
            Ax, Ay = A[:, 0:1], A[:, 1:2]
            det = Ay * B[None, :, 0] + (-Ax) * B[None, :, 1]
            alpha = (C[..., 1] * B[None, :, 0] + (-C[..., 0]) * B[None, :, 1]) / det
            beta = (C[..., 1] * Ax + (-C[..., 0]) * Ay) / det
            hit = (0 < alpha) & (alpha < 1) & (0 < beta) & (beta < 1)
            move = live & hit.any(1)
            if not move.any():
                break
            j = np.argmin(np.where(hit, alpha, np.inf), axis=1)
            al = alpha[np.arange(len(o)), j]
            Bj = B[j]
            cross = al[:, None] * r + (f32(1) - al)[:, None] * o
            s = -(Bj[:, 1] * A[:, 0] + (-Bj[:, 0]) * A[:, 1])
            nx, ny = s * A[:, 1], s * (-A[:, 0])
            nn = _norm(nx, ny)
            new = cross + f32(clearance) * np.stack((nx / nn, ny / nn), -1)
            r = np.where(move[:, None], new, r).astype(np.float32)
            iters += move
            live = move
    return r, iters


def nearest_entry(q, entries):
    """(n,) index of the entry whose points come nearest each q (n, 2)."""
    diff = q[:, None, None, :] - entries[None]
    dist = _norm(diff[..., 0], diff[..., 1]).min(-1)
    return np.argmin(dist, axis=1)


def step(state, a_next, entries, dt, radius=1.0):
    """Integrate / arrive / retire of one frame for the present agents of `state` (dict of numpy arrays: p, v, a, dest,
    flag, mask (cap), waypoints (D, cap, 2), exit_idx (D, cap)); returns the new dict (spawning not included)."""
    s = {k: np.array(v) for k, v in state.items()}
    live = s['mask'] == 1
    dtf = f32(dt)
    vn = s['v'] + s['a'] * dtf
    pn = s['p'] + s['v'] * dtf
    idx = np.nonzero(live)[0]
    flag = s['flag'].copy()
    D = s['waypoints'].shape[0]
    for i in idx:
        d = s['dest'][i]
        near = _norm(pn[i, 0] - d[0], pn[i, 1] - d[1]) < radius
        e = entries[s['exit_idx'][flag[i], i]]
        near = near or bool((_norm(pn[i, 0] - e[:, 0], pn[i, 1] - e[:, 1]) < radius).any())
        flag[i] += int(near)
    nan = np.float32(np.nan)
    gone = np.zeros_like(live)
    newdest = np.full_like(s['dest'], nan)
    for i in idx:
        if flag[i] >= D or np.isnan(s['waypoints'][flag[i], i]).any():
            gone[i] = True
        else:
            newdest[i] = s['waypoints'][flag[i], i]
    out = dict(s)
    keep = live & ~gone
    out['p'] = np.where(keep[:, None], pn, np.where(live[:, None], nan, s['p'])).astype(np.float32)
    out['v'] = np.where(keep[:, None], vn, np.where(live[:, None], 0, s['v'])).astype(np.float32)
    out['a'] = np.where(keep[:, None], a_next, np.where(live[:, None], 0, s['a'])).astype(np.float32)
    out['dest'] = np.where(live[:, None], newdest, s['dest']).astype(np.float32)
    out['flag'] = np.where(live, flag, s['flag'])
    out['mask'] = np.where(gone, 0, s['mask']).astype(np.float32)
    return out
