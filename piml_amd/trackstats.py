"""Track statistics of crowds: what an agent does along its own track, without pairing a simulated agent
with a recorded one.  The siblings (crowdstats, pairstats, flowstats) look at one frame, or two, and forget who is who; a
run can pass all three while every agent jitters, wanders, stops and restarts, or takes twice the recorded time to cross.
Four Lagrangian observables: the autocorrelation of the heading over time A(tau) with its persistence time, the mean
squared displacement MSD(tau) with its exponent (2 ballistic, 1 diffusive), the distribution of the frame-to-frame
acceleration, and per track its duration, mean speed and straightness (net displacement / path length).  The lag sweep runs
in one HIP call for all members (ops_metrics.track_stats_frames, piml_track_stats).

    python -m piml_amd.trackstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--frames a:b] [--lags 128]
                                  [--out tracks.json]

Definitions.  Slot n of a member is one agent for the whole run (a recorded clip has one pedestrian per column), so a track
is a column of P (S, T, N, 2) and M (S, T, N); velocities are not an input: every quantity comes from positions.  Agent i
takes part at (member s, frame t) when its mask is 1 and both coordinates are finite and below 65536 in magnitude (slots at
or past n_active[s] are not swept).  float32, Q = 2^20, t an index into the window [a, b) of T' frames, dt seconds per frame:
  a step (i, t) exists when i takes part at t and t + 1: u = p(t+1) - p(t), l = sqrt(ux^2 + uy^2); it is a mover when
      l / dt >= v_min, with the heading h = u / l.  Gaps are allowed: nothing requires presence between two compared frames;
  ac_n, ac_sum (S, n_lags): lag L = 1 .. n_lags, every t where steps t and t + L are movers: the pairs and the sum of
      llrintf((h_t.h_{t+L}) Q);
  msd_n, msd_sum, msd_far (S, n_lags): every t where i takes part at t and t + L, d2 = |p(t+L) - p(t)|^2: with
      sqrt(d2) < d_max the pairs and the sum of llrintf(d2 Q), otherwise msd_far counts it;
  acc (S, acc_bins + 1), acc_sum (S): every t where steps t and t + 1 exist, a = sqrt(|u_{t+1} - u_t|^2) / dt / dt, by
      floor(a / acc_bin) (the last bin is open), and the sum of llrintf(a Q) over the items below acc_bin * acc_bins;
  trk_frames, trk_steps, trk_first, trk_last, trk_path, trk_net (S, N): per track the frames taking part, the steps, the
      first and last participating frame (-1 without one), sum llrintf(l Q), and llrintf(|p(last) - p(first)| Q).
The host bins the track rows, in integer and float64 arithmetic on the integer rows only: dur_hist, speed_hist,
straight_hist (S, 2, bins) and straight_n, straight_sum (S, 2) -- index 0 every track with at least one step, index 1 the
complete tracks, first > 0 and last < T' - 1 (entered and left inside the window): the duration trk_frames dt by dur_bin,
the mean speed trk_path / (Q trk_steps dt) by speed_bin (both clipped into the last bin), the straightness trk_net /
trk_path by 1 / straight_bins (clipped into the last bin at 1: across a hole the net displacement can exceed the path;
tracks with trk_path == 0 are left out), and the sum of min((trk_net Q + trk_path // 2) // trk_path, Q)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _count, _f32, _json_float, _json_floats, _l1, _load, _nan_div, _positive, _total,
                         _window, member_indices, parse_frames)

JSON_VERSION = 1
Q = 1 << 20
LAG_ROWS = ('ac_n', 'ac_sum', 'msd_n', 'msd_sum', 'msd_far')
TRACK_ROWS = ('trk_frames', 'trk_steps', 'trk_first', 'trk_last', 'trk_path', 'trk_net')
HISTS = ('dur_hist', 'speed_hist', 'straight_hist', 'straight_n', 'straight_sum')
ADDITIVE = LAG_ROWS + ('acc', 'acc_sum') + HISTS
ARRAYS = ADDITIVE + TRACK_ROWS
# what a comparison needs equal
OPTION_KEYS = ('dt', 'v_min', 'n_lags', 'd_max', 'acc_bin', 'acc_bins', 'speed_bin', 'speed_bins', 'dur_bin', 'dur_bins',
               'straight_bins')
TRACKS = {'all': 0, 'complete': 1}


def check_options(dt=0.08, v_min=0.1, n_lags=128, d_max=64.0, acc_bin=0.25, acc_bins=40, speed_bin=0.1, speed_bins=40,
                  dur_bin=1.0, dur_bins=60, straight_bins=20, frames=None, T=None, N=None):
    """ValueError on a bad option; returns frames (a, b) or None."""
    from .ops_metrics import TRACK_MAX_BINS, TRACK_MAX_D, TRACK_MAX_FRAMES, TRACK_MAX_LAGS, TRACK_MAX_N
    for name, x in (('dt', dt), ('v_min', v_min), ('d_max', d_max), ('acc_bin', acc_bin), ('speed_bin', speed_bin),
                    ('dur_bin', dur_bin)):
        _positive(name, x)
    if _f32(d_max) > TRACK_MAX_D:
        raise ValueError(f'd_max {d_max} is beyond {TRACK_MAX_D:g} m')
    _count('n_lags', n_lags, TRACK_MAX_LAGS)
    _count('acc_bins', acc_bins, TRACK_MAX_BINS)
    for name, x in (('speed_bins', speed_bins), ('dur_bins', dur_bins), ('straight_bins', straight_bins)):
        _count(name, x, 1 << 16)
    frames = _window(frames, T)
    if T is not None and ((frames[1] - frames[0]) if frames is not None else T) > TRACK_MAX_FRAMES:
        raise ValueError(f'track_stats: a window of more than {TRACK_MAX_FRAMES} frames')
    if N is not None:
        if N > TRACK_MAX_N:
            raise ValueError(f'track_stats: {N} slots per frame (at most {TRACK_MAX_N})')
        span = (frames[1] - frames[0]) if frames is not None else (T or 0)
        top = max(_f32(d_max) ** 2, _f32(_f32(acc_bin) * int(acc_bins)))
        if not top * Q * N * span < 2.0 ** 63:
            raise ValueError(f'track_stats: {N} slots x {span} frames could overflow the 64-bit sums at d_max {d_max}, '
                             f'acc_bin * acc_bins {acc_bin * acc_bins}')
    return frames


def track_histograms(rows, Tp, dt, speed_bin=0.1, speed_bins=40, dur_bin=1.0, dur_bins=60, straight_bins=20):
    """The host half: dur_hist, speed_hist, straight_hist (S, 2, bins) and straight_n, straight_sum (S, 2) int64 from the six
    (S, N) int64 track rows of a window of Tp frames (module docstring); dt, speed_bin and dur_bin are rounded to float32
    first, as the device's options are."""
    fr, st, first, last, path, net = (np.asarray(rows[k], np.int64) for k in TRACK_ROWS)
    S = fr.shape[0]
    dt, speed_bin, dur_bin = _f32(dt), _f32(speed_bin), _f32(dur_bin)
    out = dict(dur_hist=np.zeros((S, 2, dur_bins), np.int64), speed_hist=np.zeros((S, 2, speed_bins), np.int64),
               straight_hist=np.zeros((S, 2, straight_bins), np.int64), straight_n=np.zeros((S, 2), np.int64),
               straight_sum=np.zeros((S, 2), np.int64))
    for s in range(S):
        has = st[s] > 0
        complete = has & (first[s] > 0) & (last[s] < Tp - 1)
        for k, sel in enumerate((has, complete)):
            f, n, p, d = fr[s][sel], st[s][sel], path[s][sel], net[s][sel]
            dur = np.minimum(np.floor(f.astype(np.float64) * dt / dur_bin), dur_bins - 1).astype(np.int64)
            np.add.at(out['dur_hist'][s, k], dur, 1)
            speed = p.astype(np.float64) / (float(Q) * n.astype(np.float64) * dt)
            np.add.at(out['speed_hist'][s, k], np.minimum(np.floor(speed / speed_bin), speed_bins - 1).astype(np.int64), 1)
            moved = p > 0
            p, d = p[moved], d[moved]
            np.add.at(out['straight_hist'][s, k], np.minimum(d * straight_bins // p, straight_bins - 1), 1)
            out['straight_n'][s, k] = int(moved.sum())
            out['straight_sum'][s, k] = int(np.minimum((d * Q + p // 2) // p, Q).sum())
    return out


class TrackStats:
    """The track statistics of S members (numpy int64): ac_n, ac_sum, msd_n, msd_sum, msd_far (S, n_lags); acc
    (S, acc_bins + 1); acc_sum (S); dur_hist, speed_hist, straight_hist (S, 2, bins) and straight_n, straight_sum (S, 2) made
    on the host from the track rows trk_frames, trk_steps, trk_first, trk_last, trk_path, trk_net (S, N), which are kept as
    they come from the device (None once statistics are pooled or merged: tracks of different members do not add).
    options: dt, v_min, n_lags, d_max, acc_bin, acc_bins, speed_bin, speed_bins, dur_bin, dur_bins, straight_bins, frames
    (None once statistics of different windows are merged).  The derived quantities are those of the statistics pooled over
    the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.int64))
        self.options = dict(options)

    @property
    def members(self):
        return self.ac_n.shape[0]

    @property
    def step(self):
        return float(np.float32(self.options['dt']))

    @property
    def lag_times(self):
        """(n_lags,) tau = L dt of lag L = 1 .. n_lags, seconds"""
        return np.arange(1, self.options['n_lags'] + 1, dtype=np.float64) * self.step

    def member(self, m):
        """Member m as a one-member TrackStats (views)."""
        pick = lambda x: None if x is None else x[m:m + 1]
        return TrackStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        pick = lambda x: None if x is None else x[idx]
        return TrackStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members, added in member order: a one-member TrackStats without track rows."""
        return TrackStats({k: _total(getattr(self, k)) for k in ADDITIVE}, self.options)

    @staticmethod
    def merge(stats):
        """Several TrackStats with the same options (frames aside) as one member: each pooled, added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def heading_autocorrelation(self, min_count=50):
        """(n_lags,) A(tau) = ac_sum / (Q ac_n): the mean h_t.h_{t+L} of the mover pairs L frames apart; NaN where a lag holds
        fewer than min_count pairs"""
        p = self.pooled()
        n = p.ac_n[0]
        ok = (n >= min_count) & (n > 0)
        return np.where(ok, p.ac_sum[0] / (float(Q) * np.where(ok, n, 1)), np.nan)

    def persistence_time(self, min_count=50):
        """The time at which A(tau) first falls below 1 / e: over the valid lags in order, the first tau with A < 1 / e,
        linearly interpolated from the valid lag before it (that tau itself when there is none); NaN when A never falls
        below."""
        c, tau = self.heading_autocorrelation(min_count), self.lag_times
        level, prev = 1.0 / math.e, None
        for k in np.nonzero(np.isfinite(c))[0]:
            if c[k] < level:
                if prev is None:
                    return float(tau[k])
                return float(tau[prev] + (c[prev] - level) / (c[prev] - c[k]) * (tau[k] - tau[prev]))
            prev = k
        return float('nan')

    def msd(self, min_count=50):
        """(n_lags,) MSD(tau) = msd_sum / (Q msd_n) in m^2 over the pairs closer than d_max; NaN below min_count pairs"""
        p = self.pooled()
        n = p.msd_n[0]
        ok = (n >= min_count) & (n > 0)
        return np.where(ok, p.msd_sum[0] / (float(Q) * np.where(ok, n, 1)), np.nan)

    def msd_exponent(self, min_count=50, tau_range=(0.5, 5.0)):
        """The least-squares slope of ln MSD on ln tau over the valid lags with tau_range[0] <= tau <= tau_range[1] and
        MSD > 0: 2 is ballistic, 1 diffusive; NaN with fewer than two such lags."""
        m, tau = self.msd(min_count), self.lag_times
        ok = np.isfinite(m) & (tau >= tau_range[0]) & (tau <= tau_range[1])
        ok &= np.where(ok, m, 1) > 0
        if ok.sum() < 2:
            return float('nan')
        x, y = np.log(tau[ok]), np.log(m[ok])
        x = x - x.mean()
        return float((x * (y - y.mean())).sum() / (x * x).sum())

    def acceleration_density(self):
        """(acc_bins + 1,) the share of the acceleration items per bin of acc_bin m/s^2 (the last bin is open); NaN without
        items"""
        a = self.pooled().acc[0]
        return _nan_div(a, np.full(a.shape, float(a.sum())))

    def mean_acceleration(self):
        """acc_sum / (Q items) over the items below acc_bin * acc_bins, m/s^2"""
        p = self.pooled()
        return float(_nan_div(p.acc_sum[0], float(Q) * float(p.acc[0, :-1].sum())))

    def _density(self, name, tracks):
        if tracks not in TRACKS:
            raise ValueError(f"tracks must be 'all' or 'complete', got {tracks!r}")
        h = getattr(self.pooled(), name)[0, TRACKS[tracks]]
        return _nan_div(h, np.full(h.shape, float(h.sum())))

    def duration_density(self, tracks='all'):
        """(dur_bins,) the share of tracks per bin of dur_bin seconds of trk_frames dt (the last bin takes the longer ones)"""
        return self._density('dur_hist', tracks)

    def speed_density(self, tracks='all'):
        """(speed_bins,) the share of tracks per bin of speed_bin m/s of the mean speed path / (steps dt)"""
        return self._density('speed_hist', tracks)

    def straightness_density(self, tracks='all'):
        """(straight_bins,) the share of the tracks that moved per bin of net / path in 0 .. 1"""
        return self._density('straight_hist', tracks)

    def mean_straightness(self, tracks='all'):
        """the mean net / path of the tracks that moved"""
        if tracks not in TRACKS:
            raise ValueError(f"tracks must be 'all' or 'complete', got {tracks!r}")
        p, k = self.pooled(), TRACKS[tracks]
        return float(_nan_div(p.straight_sum[0, k], float(Q) * float(p.straight_n[0, k])))

    def summary(self, min_count=50):
        p = self.pooled()
        return {'lag_times': self.lag_times.tolist(),
                'heading_autocorrelation': _json_floats(self.heading_autocorrelation(min_count)),
                'persistence_time': _json_float(self.persistence_time(min_count)), 'msd': _json_floats(self.msd(min_count)),
                'msd_exponent': _json_float(self.msd_exponent(min_count)),
                'mean_acceleration': _json_float(self.mean_acceleration()),
                'acceleration_density': _json_floats(self.acceleration_density()),
                'mean_straightness': _json_float(self.mean_straightness()),
                'mean_straightness_complete': _json_float(self.mean_straightness('complete')),
                'tracks': int(p.dur_hist[0, 0].sum()), 'complete_tracks': int(p.dur_hist[0, 1].sum()),
                'acc_items': int(p.acc.sum()), 'msd_far': int(p.msd_far.sum())}

    def to_json(self, path=None, min_count=50):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION,
             'options': {**o, 'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary(min_count)}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A TrackStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'track stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several TrackStats with the same options (frames aside) as one member: each pooled, added in list order; no track
    rows."""
    if not stats:
        raise ValueError('merge: no statistics')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in OPTION_KEYS):
            raise ValueError('merge: the statistics were taken with different options')
    pools = [s.pooled() for s in stats]
    arrays = {}
    for k in ADDITIVE:
        acc = getattr(pools[0], k).copy()
        for p in pools[1:]:
            acc += getattr(p, k)
        arrays[k] = acc
    opts = dict(stats[0].options)
    if any(s.options.get('frames') != opts.get('frames') for s in stats[1:]):
        opts['frames'] = None
    return TrackStats(arrays, opts)


def track_stats(P, M, dt=0.08, v_min=0.1, n_lags=128, d_max=64.0, acc_bin=0.25, acc_bins=40, frames=None, n_active=None,
                speed_bin=0.1, speed_bins=40, dur_bin=1.0, dur_bins=60, straight_bins=20):
    """The track statistics of positions P (S, T, N, 2) and presence M (S, T, N) -- (T, N, .) is one member -- in one device
    call for all members: TrackStats.  dt the seconds per frame; frames (a, b) the window; n_active (S) ints: member s's
    slots at or past n_active[s] never held an agent and are not swept."""
    from . import ops_metrics
    dev = next((x.device for x in (P, M) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device('cuda'))
    P, M = torch.as_tensor(P), torch.as_tensor(M)
    if P.dim() == 3:
        P, M = P[None], M[None]
    if P.dim() != 4 or P.shape[-1] != 2 or tuple(M.shape) != tuple(P.shape[:3]):
        raise ValueError(f'expected P (S, T, N, 2) or (T, N, 2) and M (S, T, N) or (T, N), got {tuple(P.shape)}, '
                         f'{tuple(M.shape)}')
    if min(P.shape[:3]) < 1:
        raise ValueError(f'empty input {tuple(P.shape)}')
    S, T, N = P.shape[:3]
    frames = check_options(dt, v_min, n_lags, d_max, acc_bin, acc_bins, speed_bin, speed_bins, dur_bin, dur_bins,
                           straight_bins, frames, T, N) or (0, T)
    P, M = (x.to(device=dev, dtype=torch.float32).contiguous() for x in (P, M))
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.track_stats_frames(P, M, dt, v_min, int(n_lags), d_max, acc_bin, int(acc_bins), frames, n_active)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host.update(track_histograms(host, frames[1] - frames[0], dt, speed_bin, int(speed_bins), dur_bin, int(dur_bins),
                                 int(straight_bins)))
    opts = dict(dt=float(dt), v_min=float(v_min), n_lags=int(n_lags), d_max=float(d_max), acc_bin=float(acc_bin),
                acc_bins=int(acc_bins), speed_bin=float(speed_bin), speed_bins=int(speed_bins), dur_bin=float(dur_bin),
                dur_bins=int(dur_bins), straight_bins=int(straight_bins), frames=frames)
    return TrackStats(host, opts)


def track_stats_of_raw(raw_data, **kw):
    """track_stats of a loaded clip (piml_amd.data.data.RawData: position, mask_p), one member; dt is the clip's time_unit
    unless given."""
    kw.setdefault('dt', float(raw_data.time_unit))
    return track_stats(raw_data.position, raw_data.mask_p, **kw)


def compare_track_stats(a, b, min_count=50):
    """Distances between two TrackStats, each pooled over its members:
      heading_ac_max_diff = max |A_a(tau) - A_b(tau)| over the lags valid in both (NaN when none; heading_ac_bins says how
          many);
      persistence_time_diff, msd_exponent_diff, mean_acceleration_diff = a's minus b's;
      acc_l1, straightness_l1, speed_l1, duration_l1 = sum |share_a - share_b| over the bins (0 .. 2; every track with a step).
    ValueError when the two were taken with different options (dt, v_min, the lags, d_max, any bin set)."""
    for k in OPTION_KEYS:
        if a.options[k] != b.options[k]:
            raise ValueError(f'compare_track_stats: the options differ ({k}: {a.options[k]} vs {b.options[k]})')
    ca, cb = a.heading_autocorrelation(min_count), b.heading_autocorrelation(min_count)
    both = np.isfinite(ca) & np.isfinite(cb)
    return {'heading_ac_max_diff': float(np.abs(ca - cb)[both].max()) if both.any() else float('nan'),
            'heading_ac_bins': int(both.sum()),
            'persistence_time_diff': a.persistence_time(min_count) - b.persistence_time(min_count),
            'msd_exponent_diff': a.msd_exponent(min_count) - b.msd_exponent(min_count),
            'acc_l1': _l1(a.acceleration_density(), b.acceleration_density()),
            'mean_acceleration_diff': a.mean_acceleration() - b.mean_acceleration(),
            'straightness_l1': _l1(a.straightness_density(), b.straightness_density()),
            'speed_l1': _l1(a.speed_density(), b.speed_density()),
            'duration_l1': _l1(a.duration_density(), b.duration_density())}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='track statistics (heading persistence, MSD, acceleration, path shape)')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--dt', type=float, default=None, help="seconds per frame (default: each clip's time_unit)")
    p.add_argument('--v_min', type=float, default=0.1)
    p.add_argument('--lags', type=int, default=128)
    p.add_argument('--d_max', type=float, default=64.0)
    p.add_argument('--acc_bin', type=float, default=0.25)
    p.add_argument('--acc_bins', type=int, default=40)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(0.08 if args.dt is None else args.dt, args.v_min, args.lags, args.d_max, args.acc_bin, args.acc_bins,
                      frames=args.frames)
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_track_stats(stats, tag, min_count=50, file=sys.stdout):
    c, m, tau = stats.heading_autocorrelation(min_count), stats.msd(min_count), stats.lag_times
    print(f'[trackstats] {tag}: A(tau), MSD(tau) (lags with >= {min_count} pairs; every lag up to 8, then powers of two)',
          file=file)
    for k in np.nonzero(np.isfinite(c) | np.isfinite(m))[0]:
        L = k + 1
        if L <= 8 or L & (L - 1) == 0 or L == len(tau):
            print(f'  tau {tau[k]:6.2f} s: A {c[k]:+.4f}  MSD {m[k]:9.4f} m^2', file=file)
    p = stats.pooled()
    print(f'[trackstats] {tag}: persistence time {stats.persistence_time(min_count):.3f} s, MSD exponent '
          f'{stats.msd_exponent(min_count):.3f}, mean acceleration {stats.mean_acceleration():.4f} m/s^2 over '
          f'{int(p.acc.sum())} items, mean straightness {stats.mean_straightness():.4f} over {int(p.straight_n[0, 0])} tracks '
          f'({stats.mean_straightness("complete"):.4f} over {int(p.straight_n[0, 1])} complete ones), '
          f'{int(p.msd_far.sum())} pairs beyond d_max', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    kw = dict(v_min=args.v_min, n_lags=args.lags, d_max=args.d_max, acc_bin=args.acc_bin, acc_bins=args.acc_bins,
              frames=args.frames)
    if args.dt is not None:
        kw['dt'] = args.dt
    data = merge([track_stats_of_raw(r, **kw) for r in raws])
    print_track_stats(data, 'data', args.min_count)
    out = {'data': data.to_json(min_count=args.min_count)}
    if ref is not None:
        rs = track_stats_of_raw(ref, **kw)
        print_track_stats(rs, 'ref', args.min_count)
        cmp = compare_track_stats(data, rs, args.min_count)
        print('[trackstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                      for k, v in cmp.items()))
        out['ref'] = rs.to_json(min_count=args.min_count)
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[trackstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
