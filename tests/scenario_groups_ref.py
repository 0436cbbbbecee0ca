"""numpy restatement of the grouped clip law of the MLAPM scenario frame (PIML_SPAWN_CLIP_GROUPS,
piml_scenario_step_mlapm_groups; piml_amd/csrc/scenario.hip, groups.hpp) for the tests: the unit rules of
`scenarios.clip_scenario(groups=)`, a frame-by-frame replay of the spawns, and the group force.

  units of a clip          tracks not seen in the window leave their group; a group left with one member is a single; a
                           single's frame f_u is its first in-window frame, a group's the first frame of the window at
                           which all its members are present (none: singles); groups of more than 4 are cut in ascending
                           track order into consecutive units of at most 4 at the group's f_u; units with f_u == a are the
                           initial ones, the others arrive; each list ordered by its units' smallest track
  unit count of frame f    the scene rules' stream: philox(f lo, f hi, 0, 0x5CE10000) word 0 >> 8 against the thresholds
  unit j of frame f        philox(f lo, f hi, j, 0x5CE30001): u = ((w0 >> 8) * Ua) >> 24 in integers, first row
                           unit_rows[u], size row_unit[first][1], one offset jitter * (2 u(w1) - 1, 2 u(w2) - 1) for the
                           whole unit (no add at jitter 0), u(w) = (w >> 8) 2^-24
  slots                    base_j = n + the sizes of units 0 .. j-1; member q: row first + q into slot base_j + q, dropped
                           from the capacity on; group_first = base_j, group_size = size for every written member
  group force              n present mates of [first, first + size) clamped to [0, rows); c = sum / n, e = c - p_i, d =
                           sqrt(ex ex + ey ey), G = d > dist (n - 1) ? (A e) / d : 0, every operation a float32 one
"""
import numpy as np

from philox_ref import philox4x32_10
from scenario_clip_ref import desired_speed
from scenario_synth_ref import spawn_counts

STREAM = 0x5CE30000
MAX_GROUP = 4
f32 = np.float32
U24 = f32(2.0 ** -24)


def units(present, groups, frames=None):
    """(initial, arrivals): lists of (tracks ascending, f_u) of the presence matrix `present` (T, N) bool over the window
    frames = (a, b), the groups given as lists of track indices; plus the counts (never_together, cut)."""
    T, N = present.shape
    a, b = (0, T) if frames is None else frames
    win = present[a:b]
    seen = win.any(0)
    first = a + win.argmax(0)
    out, grouped, apart, cut = [], set(), 0, 0
    for g in groups:
        g = sorted(i for i in g if seen[i])
        if len(g) < 2:
            continue
        together = np.nonzero(win[:, g].all(1))[0]
        if not len(together):
            apart += 1
            continue
        cut += len(g) > MAX_GROUP
        out += [(g[k:k + MAX_GROUP], a + int(together[0])) for k in range(0, len(g), MAX_GROUP)]
        grouped.update(g)
    out += [([i], int(first[i])) for i in range(N) if seen[i] and i not in grouped]
    out.sort(key=lambda u: u[0][0])
    return [u for u in out if u[1] == a], [u for u in out if u[1] != a], (apart, cut)


def table(raw, groups, frames=None, skip_frames=25):
    """(table (E, 3 + D, 2) float32, row_unit (E, 2), unit_rows (Ua), n_initial, tracks (E), frames (E)) of the RawData
    `raw`, row by row."""
    pos, vel = raw.position.numpy(), raw.velocity.numpy()
    msk, way, didx = raw.mask_p.numpy() == 1, raw.waypoints.numpy(), raw.dest_idx.numpy()
    D = way.shape[0]
    initial, arrivals, _ = units(msk, groups, frames)
    rows = [(i, f, q, len(u)) for u, f in initial + arrivals for q, i in enumerate(u)]
    v0 = desired_speed(vel, skip_frames)
    out = np.full((len(rows), 3 + D, 2), np.nan, np.float32)
    for r, (i, f, _, _) in enumerate(rows):
        out[r, 0], out[r, 1], out[r, 2] = pos[f, i], vel[f, i], (v0[i], 0.0)
        ahead = way[didx[f, i]:, i]
        out[r, 3:3 + len(ahead)] = ahead
    n_initial = sum(len(u) for u, _ in initial)
    sizes = [len(u) for u, _ in arrivals]
    unit_rows = n_initial + np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64) if sizes else np.zeros(0, np.int64)
    return (out, np.array([(q, s) for _, _, q, s in rows], np.int32).reshape(-1, 2), unit_rows.astype(np.int32), n_initial,
            np.array([i for i, _, _, _ in rows]), np.array([f for _, f, _, _ in rows]))


def _words(seed, frame, js):
    j = np.asarray(js, dtype=np.uint64)
    zero = np.zeros_like(j)
    return philox4x32_10(zero + np.uint64(frame & 0xffffffff), zero + np.uint64(frame >> 32), j, zero + np.uint64(STREAM | 1),
                         seed & 0xffffffff, (seed >> 32) & 0xffffffff)


def units_of(seed, frame, k, n_units):
    """(unit index (k) in Python integers: exact, w1 (k), w2 (k)) of the k units of a frame."""
    w = _words(seed, frame, np.arange(k))
    return np.array([((int(x) >> 8) * n_units) >> 24 for x in w[0]], np.int64), w[1], w[2]


def _u(w):
    return (w >> np.uint32(8)).astype(np.float32) * U24


def replay(tab, row_unit, unit_rows, n_initial, seed, T, thr, capacity, jitter=0.0, initial_velocity=True):
    """A free-running simulation's spawns, frame by frame: dict of counts (T) agents per frame, unit_counts (T) units per
    frame, spawned, dropped, and for every slot that held an agent (n = min(spawned, capacity) of them) born (frame), row,
    position, velocity, waypoints (D, n, 2), desired_speed, group_first, group_size; units: one (frame, unit, base slot, size)
    per drawn unit."""
    tab, row_unit = np.asarray(tab, np.float32), np.asarray(row_unit)
    k1, _ = spawn_counts(seed, np.arange(1, T), thr, [])
    slots, drawn = [], []                                     # slots: (born, row, position, group_first, group_size)
    counts, n = [n_initial], n_initial
    for i in range(min(n_initial, capacity)):
        slots.append((0, i, tab[i, 0].copy(), i - int(row_unit[i, 0]), int(row_unit[i, 1])))
    for f in range(1, T):
        k = int(k1[f - 1])
        u, w1, w2 = units_of(seed, f, k, len(unit_rows))
        base = n
        for j in range(k):
            first = int(unit_rows[u[j]])
            size = int(row_unit[first, 1])
            drawn.append((f, int(u[j]), base, size))
            for q in range(size):
                if base + q >= capacity:
                    continue
                p = tab[first + q, 0].copy()
                if f32(jitter) != 0:
                    off = np.array([f32(jitter) * (f32(2) * _u(w1[j]) - f32(1)), f32(jitter) * (f32(2) * _u(w2[j]) - f32(1))], f32)
                    p = (p + off).astype(np.float32)
                slots.append((f, first + q, p, base, size))
            base += size
        counts.append(base - n)
        n = base
    row = np.array([s[1] for s in slots], np.int64)
    vel = tab[row, 1].copy() if initial_velocity else np.zeros((len(row), 2), np.float32)
    return dict(counts=np.array(counts, np.int64), unit_counts=np.concatenate(([0], k1)).astype(np.int64), spawned=n,
                dropped=max(0, n - capacity), born=np.array([s[0] for s in slots], np.int64), row=row,
                position=np.stack([s[2] for s in slots]).astype(np.float32), velocity=vel,
                waypoints=tab[row, 3:].transpose(1, 0, 2).copy(), desired_speed=tab[row, 2, 0].copy(),
                group_first=np.array([s[3] for s in slots], np.int32), group_size=np.array([s[4] for s in slots], np.int32),
                units=drawn)


def group_force(position, group_first, group_size, A, dist):
    """(rows, 2) float32: the group term of every row, in float32 operation by operation."""
    p = np.asarray(position, np.float32).reshape(-1, 2)
    rows = p.shape[0]
    A, dist = f32(A), f32(dist)
    out = np.zeros((rows, 2), np.float32)
    for i in range(rows):
        if np.isnan(p[i]).any():
            continue
        lo, hi = max(int(group_first[i]), 0), min(int(group_first[i]) + int(group_size[i]), rows)
        sx, sy, n = f32(0), f32(0), 0
        for j in range(lo, hi):
            if np.isnan(p[j]).any():
                continue
            sx, sy, n = f32(sx + p[j, 0]), f32(sy + p[j, 1]), n + 1
        if n < 2:
            continue
        ex, ey = f32(f32(sx / f32(n)) - p[i, 0]), f32(f32(sy / f32(n)) - p[i, 1])
        d = f32(np.sqrt(f32(f32(ex * ex) + f32(ey * ey))))
        if d > f32(dist * f32(n - 1)):
            out[i] = f32(f32(A * ex) / d), f32(f32(A * ey) / d)
    return out
