"""numpy restatement of the clip spawn law of the open-world frame (PIML_SPAWN_CLIP, piml_amd/csrc/scenario.hip) for the
tests: what `scenarios.clip_scenario` puts into the track table, and a frame-by-frame replay of the spawns.

  table row of a track     (position, velocity, (desired_speed, 0), the D waypoints from its first in-window frame on, NaN
                           padded); the tracks of the window's first frame first, then the arrival tracks, in clip order
  counts of frame f        the scene rules' stream: philox(f lo, f hi, 0, 0x5CE10000) word 0 >> 8 against the thresholds
                           (scenario_synth_ref.spawn_counts)
  agent n, call 1          philox(n lo, n hi, 0, 0x5CE20001): row = n_initial + (((w0 >> 8) * Ka) >> 24) in integers,
                           origin = row point 0 + jitter * (2 u(w1) - 1, 2 u(w2) - 1), u(w) = (w >> 8) 2^-24 (no add at
                           jitter 0); the init frame draws nothing: slot i is row i
"""
import numpy as np

from philox_ref import philox4x32_10
from scenario_synth_ref import spawn_counts

STREAM = 0x5CE20000
f32 = np.float32
U24 = f32(2.0 ** -24)


def desired_speed(velocity, skip_frames=25):
    """data.desired_speed_per_agent, looped: the mean |v| (float32, as torch.norm) over the skip_frames frames from the
    first one with |v| > 0; 0 for an agent that never moves."""
    v = np.asarray(velocity, np.float32)
    speed = np.sqrt((v * v).sum(-1, dtype=np.float32), dtype=np.float32)
    out = np.zeros(v.shape[1], np.float64)
    for i in range(v.shape[1]):
        on = np.nonzero(speed[:, i] > 0)[0]
        if len(on):
            out[i] = speed[on[0]:on[0] + skip_frames, i].astype(np.float64).mean()
    return out


def table(raw, frames=None, skip_frames=25):
    """(table (E, 3 + D, 2) float32, n_initial, agents (E) clip indices of the rows, first (E) first in-window frames)
    of the RawData `raw` over the window frames = (a, b), agent by agent."""
    pos, vel = raw.position.numpy(), raw.velocity.numpy()
    msk, way, didx = raw.mask_p.numpy() == 1, raw.waypoints.numpy(), raw.dest_idx.numpy()
    T, N, D = pos.shape[0], pos.shape[1], way.shape[0]
    a, b = (0, T) if frames is None else frames
    initial, arrivals = [], []
    for i in range(N):
        on = np.nonzero(msk[a:b, i])[0]
        if len(on):
            (initial if on[0] == 0 else arrivals).append((i, a + int(on[0])))
    rows = initial + arrivals
    v0 = desired_speed(vel, skip_frames)
    out = np.full((len(rows), 3 + D, 2), np.nan, np.float32)
    for r, (i, f) in enumerate(rows):
        out[r, 0], out[r, 1], out[r, 2] = pos[f, i], vel[f, i], (v0[i], 0.0)
        ahead = way[didx[f, i]:, i]
        out[r, 3:3 + len(ahead)] = ahead
    return out, len(initial), np.array([i for i, _ in rows]), np.array([f for _, f in rows])


def _words(seed, ordinals):
    n = np.asarray(ordinals, dtype=np.uint64)
    zero = np.zeros_like(n)
    return philox4x32_10(n & np.uint64(0xffffffff), n >> np.uint64(32), zero, zero + np.uint64(STREAM | 1),
                         seed & 0xffffffff, (seed >> 32) & 0xffffffff)


def rows_of(seed, ordinals, n_initial, E):
    """the table row of each arrival ordinal (Python integers: exact)."""
    Ka = E - n_initial
    return np.array([n_initial + (((int(w) >> 8) * Ka) >> 24) for w in _words(seed, ordinals)[0]], np.int64)


def spawn(tab, n_initial, seed, ordinals, jitter=0.0, initial_velocity=True, init=False):
    """(row, position (n, 2), velocity (n, 2), waypoints (D, n, 2), desired speed (n)) of the agents `ordinals`: arrivals,
    or with init the agents of frame 0 (ordinal i = row i)."""
    ordinals = np.asarray(ordinals, np.int64)
    tab = np.asarray(tab, np.float32)
    if init:
        row = ordinals.copy()
        pos = tab[row, 0].copy()
    else:
        row = rows_of(seed, ordinals, n_initial, tab.shape[0])
        pos = tab[row, 0].copy()
        if f32(jitter) != 0:
            w = _words(seed, ordinals)
            u = lambda x: (x >> np.uint32(8)).astype(np.float32) * U24
            off = np.stack((f32(jitter) * (f32(2) * u(w[1]) - f32(1)), f32(jitter) * (f32(2) * u(w[2]) - f32(1))), -1)
            pos = (pos + off).astype(np.float32)
    vel = tab[row, 1].copy() if initial_velocity else np.zeros((len(row), 2), np.float32)
    return row, pos, vel, tab[row, 3:].transpose(1, 0, 2).copy(), tab[row, 2, 0].copy()


def replay(tab, n_initial, seed, T, thr, capacity, jitter=0.0, initial_velocity=True):
    """A free-running simulation's spawns, frame by frame: dict of counts (T) per frame, spawned, dropped, and for every
    slot that held an agent (n = min(spawned, capacity) of them) born (frame), row, position, velocity, waypoints
    (D, n, 2), desired_speed at its spawn frame."""
    k1, _ = spawn_counts(seed, np.arange(1, T), thr, [])
    counts = np.concatenate(([n_initial], k1)).astype(np.int64)
    parts, n = [], 0
    for f in range(T):
        k = int(counts[f])
        ords = np.arange(n, min(n + k, capacity))
        if len(ords):
            parts.append((np.full(len(ords), f),) + spawn(tab, n_initial, seed, ords, jitter, initial_velocity, init=f == 0))
        n += k
    cat = lambda j, axis=0: np.concatenate([p[j] for p in parts], axis)
    return dict(counts=counts, spawned=n, dropped=max(0, n - capacity), born=cat(0), row=cat(1), position=cat(2),
                velocity=cat(3), waypoints=cat(4, 1), desired_speed=cat(5))
