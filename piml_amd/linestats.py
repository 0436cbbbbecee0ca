"""Measurement-line statistics of crowds: how many people pass a given place, and when.  The siblings
(crowdstats, pairstats, flowstats, trackstats, obstaclestats) measure fields and pairs; none counts the throughput of a
door or a cross-section, the macroscopic check a pedestrian study reports first.  Per measurement line and direction: the
N-t curve, the flow J and the specific flow J / width, the speed and the lateral position at the crossing, the time headway
between successive crossings; between two lines the travel time, whose count is the origin-destination matrix between
gates.  One HIP call for all members against one shared set of lines (ops_metrics.line_stats_frames, piml_line_stats).

    python -m piml_amd.linestats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] --lines 'auto' | 'ax,ay,bx,by;...'
                                 [--box x0,x1,y0,y1 | auto] [--frames a:b] [--out lines.json]

Definitions.  P (S, T, N, 2) and M (S, T, N) float32; velocities are not an input: as in trackstats, slot n of a member is
one agent for the whole run.  lines (L, 4) float32, each row (ax, ay, bx, by), shared by all members, 1 <= L <= 16; a row
must be finite, below 65536 in magnitude, and a != b after rounding to float32 (ValueError otherwise).  Agent i takes part
at (member s, frame t) when its mask is 1 and both coordinates are finite and below 65536 in magnitude (slots at or past
n_active[s] are not swept); t is an index into the window [a, b) of T' frames.  A step (i, t) exists when i takes part at t
and at t + 1, and t + 1 < T'.  No step spans a gap: a crossing made while the agent is absent is not seen.  float32 with
true divisions and square roots and no contraction, Q = 2^20.  Per line, d = b - a, len2 = dx dx + dy dy:
  side(p) = dx (py - ay) - dy (px - ax); for a step s0 = side(p(t)), s1 = side(p(t+1));
  direction 0 ("forward", from the right of a->b to its left) when s0 < 0 and s1 >= 0, direction 1 when s0 >= 0 and
      s1 < 0: a point exactly on the line belongs to the left side, so a touch is never counted twice;
  f = s0 / (s0 - s1), u = p(t+1) - p(t), c = p(t) + f u, w = ((cx - ax) dx + (cy - ay) dy) / len2;
  the step is a crossing of the line when 0 <= w < 1: the interval is half-open, so two collinear lines that share an end
      point count each crossing exactly once between them;
  normal speed vn = |s1 - s0| / sqrt(len2) / dt (m/s); crossing time in Q-frames tc = t Q + llrintf(f Q).
Device outputs, int64:
  cross (S, L, 2): crossings per direction; nt (S, L, 2, T'): crossings whose step starts at frame t (the N-t curve is its
      cumulative sum; entry T' - 1 is always 0);
  speed (S, L, 2, v_bins + 1): by min(floor(vn / v_bin), v_bins) (the last bin is open); speed_sum (S, L, 2): the sum of
      llrintf(vn Q) over the crossings with vn < v_bin * v_bins;
  profile (S, L, 2, w_bins): by min(floor(w w_bins), w_bins - 1);
  steps (S): the steps swept (the denominator of an ambiguity share); trk_steps (S, N): the steps of each track;
  trk_count (S, L, N): crossings of the line by the track, both directions; trk_first: the smallest tc, or -1 without a
      crossing; trk_dir: the direction of that first crossing, or -1.  The minimum is taken over 2 tc + dir, so time and
      direction come from the same step; of two crossings at the same tc (a step that ends exactly on the line, counted
      forward, and the next that leaves it backwards) direction 0 is the first.
The host half, in integer and float64 arithmetic on the integer rows only (host_rows):
  headway (S, L, 2, h_bins + 1): the tracks whose first crossing of the line has that direction, their trk_first sorted,
      the successive differences D binned by min(floor(D / Q * dt / h_bin), h_bins); headway_n, headway_sum (S, L, 2): the
      number of differences and their sum in Q-frames;
  travel (S, L, L, tt_bins + 1), travel_n, travel_sum (S, L, L): for every ordered pair l != m the tracks with a first
      crossing on both lines and trk_first[l] < trk_first[m], the difference binned by min(floor(D / Q * dt / tt_bin),
      tt_bins); the count is the origin-destination matrix between the lines;
  tracks (S): the slots with at least one step; slices (S): the frames of the window, the observed time in frames.
A re-crossing is counted in cross, nt, speed, profile and trk_count; it is not counted in headway or travel time, which
follow first crossings."""
import argparse
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _count, _f32, _json_float, _json_floats, _load, _nan_div, _positive, _total, _window,
                         auto_box, member_indices, parse_box, parse_frames)

JSON_VERSION = 1
Q = 1 << 20
MAX_COORD = 65536.0
DIR_ROWS = ('cross', 'nt', 'speed', 'speed_sum', 'profile')
TRACK_ROWS = ('trk_steps', 'trk_count', 'trk_first', 'trk_dir')
HISTS = ('headway', 'headway_n', 'headway_sum', 'travel', 'travel_n', 'travel_sum', 'tracks')
DEVICE = DIR_ROWS + ('steps',) + TRACK_ROWS
ADDITIVE = DIR_ROWS + ('steps',) + HISTS + ('slices',)
ARRAYS = ADDITIVE + TRACK_ROWS
# what a comparison needs equal (the lines are part of what was measured)
OPTION_KEYS = ('dt', 'v_bin', 'v_bins', 'w_bins', 'h_bin', 'h_bins', 'tt_bin', 'tt_bins', 'n_lines', 'lines_hash')


def check_lines(lines):
    """(L, 4) float32 contiguous numpy of a set of lines (tensor, array or list of rows ax, ay, bx, by); ValueError unless
    1 <= L <= LINE_MAX_L and every row is finite, below 65536 in magnitude and has a != b after rounding to float32."""
    from .ops_metrics import LINE_MAX_L
    if isinstance(lines, torch.Tensor):
        lines = lines.detach().cpu().numpy()
    try:
        with np.errstate(over='ignore'):
            arr = np.asarray(lines, np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f'lines: expected rows (ax, ay, bx, by), got {lines!r}') from None
    if arr.ndim == 1 and arr.size == 4:
        arr = arr[None]
    if arr.ndim != 2 or arr.shape[1] != 4:
        raise ValueError(f'lines: expected (L, 4) rows (ax, ay, bx, by), got shape {arr.shape}')
    if not 1 <= arr.shape[0] <= LINE_MAX_L:
        raise ValueError(f'lines: {arr.shape[0]} lines (1..{LINE_MAX_L})')
    for k, row in enumerate(arr):
        if not (np.isfinite(row).all() and (np.abs(row) < MAX_COORD).all()):
            raise ValueError(f'lines: row {k} {row.tolist()} is not finite and below {MAX_COORD:g} in magnitude')
        if row[0] == row[2] and row[1] == row[3]:
            raise ValueError(f'lines: row {k} {row.tolist()} is degenerate (a == b)')
    return np.ascontiguousarray(arr)


def lines_hash(lines):
    """sha256 of the float32 bytes of the (L, 4) lines, hex"""
    return hashlib.sha256(check_lines(lines).tobytes()).hexdigest()


def auto_lines(box):
    """Two lines of a box (x0, x1, y0, y1): its vertical mid-line from bottom to top (direction 0: leftwards, towards -x)
    and its horizontal mid-line from left to right (direction 0: upwards, towards +y); (2, 4) float32."""
    x0, x1, y0, y1 = (float(v) for v in box)
    if not (all(math.isfinite(v) for v in (x0, x1, y0, y1)) and x0 < x1 and y0 < y1):
        raise ValueError(f'auto_lines: box {tuple(box)} is empty or not finite (need x0 < x1 and y0 < y1)')
    xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    return check_lines([[xm, y0, xm, y1], [x0, ym, x1, ym]])


def parse_lines(text):
    """'ax,ay,bx,by;ax,ay,bx,by;...' -> (L, 4) float32 (checked); 'auto' -> 'auto'."""
    text = text.strip()
    if text == 'auto':
        return 'auto'
    rows = []
    for part in (q for q in text.split(';') if q.strip()):
        try:
            vals = [float(v) for v in part.split(',')]
        except ValueError:
            raise ValueError(f'expected ax,ay,bx,by, got {part!r}') from None
        if len(vals) != 4:
            raise ValueError(f'expected ax,ay,bx,by, got {part!r}')
        rows.append(vals)
    if not rows:
        raise ValueError(f'no line in {text!r}')
    return check_lines(rows)


def check_options(dt=0.08, v_bin=0.1, v_bins=40, w_bins=16, h_bin=0.25, h_bins=80, tt_bin=1.0, tt_bins=60, frames=None,
                  T=None, N=None):
    """ValueError on a bad option; returns frames (a, b) or None."""
    from .ops_metrics import LINE_MAX_BINS, LINE_MAX_FRAMES, LINE_MAX_N
    for name, x in (('dt', dt), ('v_bin', v_bin), ('h_bin', h_bin), ('tt_bin', tt_bin)):
        _positive(name, x)
    for name, x in (('v_bins', v_bins), ('w_bins', w_bins), ('h_bins', h_bins), ('tt_bins', tt_bins)):
        _count(name, x, LINE_MAX_BINS)
    frames = _window(frames, T)
    span = (frames[1] - frames[0]) if frames is not None else (T or 0)
    if span > LINE_MAX_FRAMES:
        raise ValueError(f'line_stats: {span} frames in the window (at most {LINE_MAX_FRAMES})')
    if N is not None:
        if N > LINE_MAX_N:
            raise ValueError(f'line_stats: {N} slots per frame (at most {LINE_MAX_N})')
        top = _f32(_f32(v_bin) * int(v_bins))
        if not (math.isfinite(top) and top * Q * N * span < 2.0 ** 63):
            raise ValueError(f'line_stats: {N} slots x {span} frames could overflow the 64-bit speed sum '
                             f'(v_bin * v_bins {v_bin * v_bins})')
    return frames


def host_rows(rows, dt=0.08, h_bin=0.25, h_bins=80, tt_bin=1.0, tt_bins=60):
    """The host half: headway (S, L, 2, h_bins + 1), headway_n, headway_sum (S, L, 2), travel (S, L, L, tt_bins + 1),
    travel_n, travel_sum (S, L, L) and tracks (S) int64 from the track rows trk_steps (S, N), trk_first and trk_dir
    (S, L, N) (module docstring); dt, h_bin and tt_bin are rounded to float32 first, as the device's options are."""
    steps, first, dirs = (np.asarray(rows[k], np.int64) for k in ('trk_steps', 'trk_first', 'trk_dir'))
    S, L, _ = first.shape
    dt, h_bin, tt_bin, HB, TB = _f32(dt), _f32(h_bin), _f32(tt_bin), int(h_bins), int(tt_bins)
    out = dict(headway=np.zeros((S, L, 2, HB + 1), np.int64), headway_n=np.zeros((S, L, 2), np.int64),
               headway_sum=np.zeros((S, L, 2), np.int64), travel=np.zeros((S, L, L, TB + 1), np.int64),
               travel_n=np.zeros((S, L, L), np.int64), travel_sum=np.zeros((S, L, L), np.int64),
               tracks=(steps > 0).sum(1).astype(np.int64))
    for s in range(S):
        for l in range(L):
            for d in (0, 1):
                tc = np.sort(first[s, l][(dirs[s, l] == d) & (first[s, l] >= 0)])
                gap = np.diff(tc)
                np.add.at(out['headway'][s, l, d],
                          np.minimum(np.floor(gap.astype(np.float64) / float(Q) * dt / h_bin), HB).astype(np.int64), 1)
                out['headway_n'][s, l, d] = gap.size
                out['headway_sum'][s, l, d] = int(gap.sum())
            for m in range(L):
                if m == l:
                    continue
                both = (first[s, l] >= 0) & (first[s, m] >= 0) & (first[s, l] < first[s, m])
                gap = (first[s, m] - first[s, l])[both]
                np.add.at(out['travel'][s, l, m],
                          np.minimum(np.floor(gap.astype(np.float64) / float(Q) * dt / tt_bin), TB).astype(np.int64), 1)
                out['travel_n'][s, l, m] = gap.size
                out['travel_sum'][s, l, m] = int(gap.sum())
    return out


class LineStats:
    """The measurement-line statistics of S members (numpy int64): cross, speed_sum (S, L, 2); nt (S, L, 2, T'); speed
    (S, L, 2, v_bins + 1); profile (S, L, 2, w_bins); steps (S); headway, headway_n, headway_sum, travel, travel_n,
    travel_sum and tracks made on the host, once per member, from the track rows trk_steps (S, N), trk_count, trk_first,
    trk_dir (S, L, N), which are kept as they come from the device (None once statistics are pooled or merged: tracks of
    different members do not add); slices (S): the frames each row observed (T' per member, more once pooled).  nt is None
    once statistics of windows of different lengths are merged.  options: dt, v_bin, v_bins, w_bins, h_bin, h_bins, tt_bin,
    tt_bins, lines (the float32 rows), n_lines, lines_hash (sha256 of their float32 bytes) and frames (None once statistics
    of different windows are merged).  The derived quantities are those of the statistics pooled over the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.int64))
        self.options = dict(options)

    @property
    def members(self):
        return self.cross.shape[0]

    @property
    def n_lines(self):
        return self.cross.shape[1]

    @property
    def lines(self):
        return np.asarray(self.options['lines'], np.float32).reshape(-1, 4)

    @property
    def dt(self):
        return _f32(self.options['dt'])

    def member(self, m):
        """Member m as a one-member LineStats (views)."""
        pick = lambda x: None if x is None else x[m:m + 1]
        return LineStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        pick = lambda x: None if x is None else x[idx]
        return LineStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members, added in member order: a one-member LineStats without track rows."""
        return LineStats({k: None if getattr(self, k) is None else _total(getattr(self, k)) for k in ADDITIVE}, self.options)

    @staticmethod
    def merge(stats):
        """Several LineStats with the same options (frames aside) as one member: each pooled, added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def line_lengths(self):
        """(L,) the lengths of the lines in metres, float64 of the float32 rows"""
        ln = self.lines.astype(np.float64)
        return np.hypot(ln[:, 2] - ln[:, 0], ln[:, 3] - ln[:, 1])

    def flow(self):
        """(L, 2) crossings per second of observed time, cross / (slices dt)"""
        p = self.pooled()
        return _nan_div(p.cross[0], np.full(p.cross[0].shape, float(p.slices[0]) * self.dt))

    def specific_flow(self):
        """(L, 2) flow per metre of line"""
        return self.flow() / self.line_lengths()[:, None]

    def n_t(self):
        """(L, 2, T') the cumulative number of crossings whose step started at or before frame t, summed over the members"""
        p = self.pooled()
        if p.nt is None:
            raise ValueError('n_t: the statistics were merged over windows of different lengths')
        return np.cumsum(p.nt[0], -1)

    def flow_series(self, window_s=5.0):
        """(L, 2, K) crossings per second and member in consecutive windows of k = max(round(window_s / dt), 1) frames (the
        K = T' // k whole ones)"""
        p = self.pooled()
        if p.nt is None:
            raise ValueError('flow_series: the statistics were merged over windows of different lengths')
        nt = p.nt[0]
        Tp = nt.shape[-1]
        k = max(int(round(float(window_s) / self.dt)), 1)
        K = Tp // k
        runs = float(p.slices[0]) / max(Tp, 1)
        return nt[..., :K * k].reshape(*nt.shape[:-1], K, k).sum(-1) / (k * self.dt * runs)

    def crossing_speed_density(self):
        """(L, 2, v_bins) crossings per crossing and per m/s of normal speed (the rest: beyond the range)"""
        c = self.pooled().speed[0]
        return _nan_div(c[..., :-1], np.broadcast_to(c.sum(-1, keepdims=True) * _f32(self.options['v_bin']), c[..., :-1].shape))

    def mean_crossing_speed(self):
        """(L, 2) speed_sum / (Q crossings) over the crossings below v_bin * v_bins, m/s"""
        p = self.pooled()
        return _nan_div(p.speed_sum[0], float(Q) * p.speed[0][..., :-1].sum(-1))

    def profile_density(self):
        """(L, 2, w_bins) crossings per crossing and per unit of the line coordinate w in [0, 1)"""
        c = self.pooled().profile[0]
        return _nan_div(c * float(c.shape[-1]), np.broadcast_to(c.sum(-1, keepdims=True), c.shape))

    def headway_density(self):
        """(L, 2, h_bins) headways per headway and per second (the rest: beyond the range)"""
        c = self.pooled().headway[0]
        return _nan_div(c[..., :-1], np.broadcast_to(c.sum(-1, keepdims=True) * _f32(self.options['h_bin']), c[..., :-1].shape))

    def mean_headway(self):
        """(L, 2) the mean time between successive first crossings, seconds (every headway, the open bin included)"""
        p = self.pooled()
        return _nan_div(p.headway_sum[0] / float(Q) * self.dt, p.headway_n[0])

    def travel_time_density(self, l, m):
        """(tt_bins,) travel times from line l to line m per travel time and per second (the rest: beyond the range)"""
        c = self.pooled().travel[0, l, m]
        return _nan_div(c[:-1], np.full(c[:-1].shape, float(c.sum()) * _f32(self.options['tt_bin'])))

    def mean_travel_time(self):
        """(L, L) the mean time from the first crossing of line l to the later first crossing of line m, seconds"""
        p = self.pooled()
        return _nan_div(p.travel_sum[0] / float(Q) * self.dt, p.travel_n[0])

    def od_counts(self):
        """(L, L) the tracks that cross line l first and line m later: the origin-destination matrix between the lines"""
        return self.pooled().travel_n[0].copy()

    def od_fraction(self):
        """(L, L) od_counts per track that crosses line l and any other line later (rows sum to 1; NaN without one)"""
        c = self.od_counts()
        return _nan_div(c, np.broadcast_to(c.sum(1, keepdims=True), c.shape))

    def summary(self):
        p = self.pooled()
        return {'lines': self.lines.astype(np.float64).tolist(), 'line_lengths': self.line_lengths().tolist(),
                'cross': p.cross[0].tolist(), 'flow': _json_floats(self.flow()), 'specific_flow': _json_floats(self.specific_flow()),
                'mean_crossing_speed': _json_floats(self.mean_crossing_speed()),
                'mean_headway': _json_floats(self.mean_headway()), 'mean_travel_time': _json_floats(self.mean_travel_time()),
                'od_counts': p.travel_n[0].tolist(), 'steps': int(p.steps[0]), 'tracks': int(p.tracks[0]),
                'slices': int(p.slices[0])}

    def to_json(self, path=None):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION,
             'options': {**o, 'lines': [list(map(float, r)) for r in o['lines']],
                         'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary()}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A LineStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'line stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['lines'] = [list(map(float, r)) for r in o['lines']]
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several LineStats with the same options (frames aside; the lines included) as one member: each pooled, added in list
    order; no track rows, and no nt when the windows differ in length."""
    if not stats:
        raise ValueError('merge: no statistics')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in OPTION_KEYS):
            raise ValueError('merge: the statistics were taken with different options or lines')
    pools = [s.pooled() for s in stats]
    same_len = all(p.nt is not None and p.nt.shape == pools[0].nt.shape for p in pools)
    arrays = {}
    for k in ADDITIVE:
        if k == 'nt' and not same_len:
            arrays[k] = None
            continue
        acc = getattr(pools[0], k).copy()
        for p in pools[1:]:
            acc += getattr(p, k)
        arrays[k] = acc
    opts = dict(stats[0].options)
    if any(s.options.get('frames') != opts.get('frames') for s in stats[1:]):
        opts['frames'] = None
    return LineStats(arrays, opts)


def _promote(P, M):
    """(T, N, .) -> (1, T, N, .); torch or numpy in, float32 contiguous on a GPU out."""
    dev = next((x.device for x in (P, M) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device('cuda'))
    P, M = torch.as_tensor(P), torch.as_tensor(M)
    if P.dim() == 3:
        P, M = P[None], M[None]
    if P.dim() != 4 or P.shape[-1] != 2 or tuple(M.shape) != tuple(P.shape[:3]):
        raise ValueError(f'expected P (S, T, N, 2) or (T, N, 2) and M (S, T, N) or (T, N), got {tuple(P.shape)}, '
                         f'{tuple(M.shape)}')
    if min(P.shape[:3]) < 1:
        raise ValueError(f'empty input {tuple(P.shape)}')
    return tuple(x.to(device=dev, dtype=torch.float32).contiguous() for x in (P, M))


def line_stats(P, M, lines, dt=0.08, v_bin=0.1, v_bins=40, w_bins=16, h_bin=0.25, h_bins=80, tt_bin=1.0, tt_bins=60,
               frames=None, n_active=None):
    """The measurement-line statistics of positions P (S, T, N, 2) and presence M (S, T, N) -- (T, N, .) is one member --
    against the lines (L, 4), rows (ax, ay, bx, by), in one device call for all members: LineStats.  dt the seconds per
    frame; frames (a, b) the window; n_active (S) ints: member s's slots at or past n_active[s] never held an agent and
    are not swept.  Every option and line is checked on the host before anything is launched."""
    from . import ops_metrics
    rows = check_lines(lines)
    shape = tuple(getattr(P, 'shape', ()))
    T, N = (shape[-3], shape[-2]) if len(shape) in (3, 4) else (None, None)
    frames = check_options(dt, v_bin, v_bins, w_bins, h_bin, h_bins, tt_bin, tt_bins, frames, T, N)
    P, M = _promote(P, M)
    S, T, N = P.shape[:3]
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.line_stats_frames(P, M, torch.from_numpy(rows).to(P.device), dt, v_bin, int(v_bins), int(w_bins),
                                        frames, n_active)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host.update(host_rows(host, dt, h_bin, int(h_bins), tt_bin, int(tt_bins)))
    host['slices'] = np.full(S, frames[1] - frames[0], np.int64)
    opts = dict(dt=float(dt), v_bin=float(v_bin), v_bins=int(v_bins), w_bins=int(w_bins), h_bin=float(h_bin),
                h_bins=int(h_bins), tt_bin=float(tt_bin), tt_bins=int(tt_bins), frames=frames,
                lines=rows.astype(np.float64).tolist(), n_lines=int(rows.shape[0]), lines_hash=lines_hash(rows))
    return LineStats(host, opts)


def line_stats_of_raw(raw_data, lines, **kw):
    """line_stats of a loaded clip (piml_amd.data.data.RawData: position, mask_p), one member; dt is the clip's time_unit
    unless given."""
    kw.setdefault('dt', float(raw_data.time_unit))
    return line_stats(raw_data.position, raw_data.mask_p, lines, **kw)


def _shares(h):
    return _nan_div(h, np.broadcast_to(h.sum(-1, keepdims=True), h.shape))


def _mean_l1(ha, hb, min_count):
    """the mean over the leading entries with at least min_count items on both sides of sum |share_a - share_b| over the last
    axis (0 .. 2); NaN without such an entry"""
    ok = (ha.sum(-1) >= min_count) & (hb.sum(-1) >= min_count) & (ha.sum(-1) > 0) & (hb.sum(-1) > 0)
    if not ok.any():
        return float('nan')
    return float(np.abs(_shares(ha[ok]) - _shares(hb[ok])).sum(-1).mean())


def compare_line_stats(a, b, min_count=50):
    """Distances between two LineStats, each pooled over its members (b is the reference side):
      flow_rel_diff = the mean over the (line, direction) entries with at least min_count crossings on the b side of
          |Ja - Jb| / Jb;
      direction_split_diff = the mean over the lines with at least min_count crossings on both sides of |share_a - share_b|
          of direction 0 among the line's crossings;
      speed_l1, profile_l1, headway_l1 = the mean over the (line, direction) entries with at least min_count items on both
          sides of sum |share_a - share_b| over the bins, the open last bin included (0 .. 2); travel_l1 the same over the
          ordered pairs of lines;
      mean_speed_diff = the mean over the same entries as speed_l1 of |mean_crossing_speed a - b|, m/s;
      mean_travel_rel_diff = the mean over the pairs of travel_l1 of |Ta - Tb| / Tb of the mean travel times.
    A term without enough data is NaN.  ValueError when the two were taken with different options (dt, any bin set) or on
    different lines (their number or float32 bytes: n_lines, lines_hash)."""
    for k in OPTION_KEYS:
        if a.options[k] != b.options[k]:
            what = 'lines' if k in ('n_lines', 'lines_hash') else 'options'
            raise ValueError(f'compare_line_stats: the {what} differ ({k}: {a.options[k]} vs {b.options[k]})')
    pa, pb = a.pooled(), b.pooled()
    ja, jb = a.flow(), b.flow()
    ok = (pb.cross[0] >= min_count) & (pb.cross[0] > 0)
    flow = float((np.abs(ja - jb)[ok] / jb[ok]).mean()) if ok.any() else float('nan')
    ta, tb = pa.cross[0].sum(-1), pb.cross[0].sum(-1)
    okl = (ta >= min_count) & (tb >= min_count) & (ta > 0) & (tb > 0)
    split = float(np.abs(pa.cross[0][okl, 0] / ta[okl] - pb.cross[0][okl, 0] / tb[okl]).mean()) if okl.any() else float('nan')
    sa, sb = pa.speed[0], pb.speed[0]
    oks = (sa.sum(-1) >= min_count) & (sb.sum(-1) >= min_count) & (sa[..., :-1].sum(-1) > 0) & (sb[..., :-1].sum(-1) > 0)
    speed = float(np.abs(a.mean_crossing_speed() - b.mean_crossing_speed())[oks].mean()) if oks.any() else float('nan')
    va, vb = pa.travel[0], pb.travel[0]
    okt = (va.sum(-1) >= min_count) & (vb.sum(-1) >= min_count) & (va.sum(-1) > 0) & (vb.sum(-1) > 0)
    ma, mb = a.mean_travel_time(), b.mean_travel_time()
    travel = float((np.abs(ma - mb)[okt] / mb[okt]).mean()) if okt.any() else float('nan')
    return {'flow_rel_diff': flow, 'direction_split_diff': split, 'speed_l1': _mean_l1(sa, sb, min_count),
            'profile_l1': _mean_l1(pa.profile[0], pb.profile[0], min_count),
            'headway_l1': _mean_l1(pa.headway[0], pb.headway[0], min_count), 'travel_l1': _mean_l1(va, vb, min_count),
            'mean_speed_diff': speed, 'mean_travel_rel_diff': travel}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='measurement-line statistics (flow, headway, crossing speed, travel time) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--lines', type=str, required=True,
                   help="'ax,ay,bx,by;ax,ay,bx,by;...' or 'auto' (the two mid-lines of --box)")
    p.add_argument('--box', type=str, default=None,
                   help="--lines auto: x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data, in 0.5 m cells)")
    p.add_argument('--dt', type=float, default=None, help="seconds per frame (default: each clip's time_unit)")
    p.add_argument('--v_bin', type=float, default=0.1)
    p.add_argument('--v_bins', type=int, default=40)
    p.add_argument('--w_bins', type=int, default=16)
    p.add_argument('--h_bin', type=float, default=0.25)
    p.add_argument('--h_bins', type=int, default=80)
    p.add_argument('--tt_bin', type=float, default=1.0)
    p.add_argument('--tt_bins', type=int, default=60)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.lines = parse_lines(args.lines)
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(0.08 if args.dt is None else args.dt, args.v_bin, args.v_bins, args.w_bins, args.h_bin, args.h_bins,
                      args.tt_bin, args.tt_bins, args.frames)
        if isinstance(args.lines, str) and args.box is None:
            raise ValueError('--lines auto needs --box (x0,x1,y0,y1 or auto)')
        if not isinstance(args.lines, str) and args.box is not None:
            raise ValueError('--box only feeds --lines auto')
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_line_stats(stats, tag, file=sys.stdout):
    p = stats.pooled()
    flow, spec, speed, head = stats.flow(), stats.specific_flow(), stats.mean_crossing_speed(), stats.mean_headway()
    print(f'[linestats] {tag}: {int(p.steps[0])} steps of {int(p.tracks[0])} tracks over {int(p.slices[0])} frames '
          f'({float(p.slices[0]) * stats.dt:g} s)', file=file)
    for l, row in enumerate(stats.lines):
        print(f'  line {l} ({row[0]:g}, {row[1]:g}) -> ({row[2]:g}, {row[3]:g}), {stats.line_lengths()[l]:.3f} m', file=file)
        for d in (0, 1):
            print(f'    direction {d}: {int(p.cross[0, l, d]):7d} crossings, J {flow[l, d]:.4f} /s, Js {spec[l, d]:.4f} /s/m, '
                  f'speed {speed[l, d]:.4f} m/s, headway {head[l, d]:.4f} s', file=file)
    od, tt = stats.od_counts(), stats.mean_travel_time()
    for l in range(od.shape[0]):
        for m in range(od.shape[1]):
            if od[l, m]:
                print(f'  line {l} -> line {m}: {int(od[l, m]):7d} tracks, mean travel time {tt[l, m]:.3f} s', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    lines = args.lines
    if isinstance(lines, str):
        box = args.box
        if box == 'auto':
            src = ref if ref is not None else raws[0]
            box = auto_box(src.position.numpy(), src.mask_p.numpy(), 0.5)
            print(f'[linestats] --box auto: {",".join(f"{v:g}" for v in box)}')
        try:
            lines = auto_lines(box)
        except ValueError as ex:
            sys.exit(f'--lines auto: {ex}')
    kw = dict(v_bin=args.v_bin, v_bins=args.v_bins, w_bins=args.w_bins, h_bin=args.h_bin, h_bins=args.h_bins,
              tt_bin=args.tt_bin, tt_bins=args.tt_bins, frames=args.frames)
    if args.dt is not None:
        kw['dt'] = args.dt
    data = merge([line_stats_of_raw(r, lines, **kw) for r in raws])
    print_line_stats(data, 'data')
    out = {'data': data.to_json()}
    if ref is not None:
        rs = line_stats_of_raw(ref, lines, **kw)
        print_line_stats(rs, 'ref')
        cmp = compare_line_stats(data, rs, args.min_count)
        print('[linestats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' for k, v in cmp.items()))
        out['ref'] = rs.to_json()
        out['compare'] = {k: _json_float(v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[linestats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
