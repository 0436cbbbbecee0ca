"""Obstacle statistics of crowds: what the agents do next to the scene's walls and pillars.  The siblings
(crowdstats, pairstats, flowstats, trackstats) compare agents with agents and never read the obstacles a scene or clip
carries; a run can pass all four while a fifth of its tracks cross a wall -- which the closed-form MLAPM law, having no
obstacle term, makes them do.  Four observables: the clearance to the nearest obstacle point with the speed at that
clearance (do agents slow down near a wall?), the contacts, the smallest time to an obstacle, and per step the clearance of
the swept segment with the crossings ("hits": tunnelling between two frames).  One HIP call for all members against one
shared obstacle set (ops_metrics.obstacle_stats_frames, piml_obstacle_stats).

    python -m piml_amd.obstaclestats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--obstacles other.npy]
                                     [--box auto] [--frames a:b] [--out walls.json]

Definitions.  P, V (S, T, N, 2) and M (S, T, N) float32; obs (O, 2) float32, shared by all members.  Agent i takes part at
(member s, frame t) when its mask is 1, both coordinates of P are finite and below 65536 in magnitude and both components
of V are finite and below 1024 in magnitude (slots at or past n_active[s] are not swept); it is focal when it takes part and
lies in the box [x0, x1) x [y0, y1), if there is one.  An obstacle point is valid when both of its coordinates are finite;
the others are skipped, and with no valid point only focal and steps count (an empty obstacle set, O = 0, is an empty
problem: every output is 0, trk_min -1).  float32 with true divisions and square roots and no contraction, Q = 2^20, t an
index into the window [a, b) of T' frames.  For a focal (i, t) and every valid point q, e = q - p(t):
  clearance r = sqrt(min_q |e|^2); a contact when r < radius (the body radius, half of pairstats' pair radius);
  time to wall, pairstats' formula for a point at rest: c = |e|^2 - radius^2, b = -(e.v), a = |v|^2; on a collision course
      when c >= 0, b < 0 and disc = b^2 - a c >= 0, then tau = c / (-b + sqrt(disc)); tau_min = min_q tau;
  swept clearance: a step (i, t) exists when i is focal at t, takes part at t + 1 and t + 1 < T'; u = p(t+1) - p(t),
      len2 = |u|^2, s = min(max((e.u) / len2, 0), 1) (s = 0 when len2 == 0), m = sqrt(min_q |e - s u|^2); a hit when
      m < hit_radius: the step's segment touches the obstacle, even when neither end is in contact.
The minima are exact in float32 whatever the order of the points, so the device reproduces a float32 numpy run bit for bit.
Outputs, int64:
  focal, steps, contact, hit (S);
  clear (S, r_bins + 1): each focal agent-frame by min(floor(r / r_bin), r_bins) (the last bin is open); clear_speed (S,
      r_bins + 1): the sum of llrintf(sqrt(|v|^2) Q) over the same items per bin; clear_sum (S): the sum of llrintf(r Q) over
      the items with r < r_bin * r_bins;
  swept (S, r_bins + 1): each step by min(floor(m / r_bin), r_bins);
  min_ttc (S, tau_bins + 1): each focal agent-frame by floor(tau_min / tau_bin) where that is below tau_bins, else (on no
      collision course, or beyond the range) bin tau_bins;
  trk_frames, trk_contacts, trk_hits, trk_min (S, N): per track its focal frames, contacts and hits, and
      llrintf(Q min(r, 2^24)) of its smallest r (-1 without a focal frame).
The host bins the track rows, in integer and float64 arithmetic on the integer rows only: trk_min_hist (S, r_bins + 1), the
tracks with a focal frame by min(floor(trk_min / Q / r_bin), r_bins), and tracks, tracks_hit, tracks_contact (S): the
tracks with at least one focal frame, one hit, one contact.  dt (seconds per frame) scales no device quantity (velocities
are an input); it is recorded, and two statistics taken at different dt do not compare: a step is dt long."""
import argparse
import hashlib
import json
import math
import os
import sys
import warnings

import numpy as np
import torch

from .crowdstats import (_bounds, _count, _f32, _json_float, _json_floats, _l1, _load, _nan_div, _positive, _promote,
                         _total, _window, auto_box, member_indices, parse_box, parse_frames)

JSON_VERSION = 1
Q = 1 << 20
COUNTS = ('focal', 'steps', 'contact', 'hit', 'clear_sum')
R_ROWS = ('clear', 'clear_speed', 'swept')
TRACK_ROWS = ('trk_frames', 'trk_contacts', 'trk_hits', 'trk_min')
HISTS = ('trk_min_hist', 'tracks', 'tracks_hit', 'tracks_contact')
DEVICE = COUNTS + R_ROWS + ('min_ttc',) + TRACK_ROWS
ADDITIVE = COUNTS + R_ROWS + ('min_ttc',) + HISTS
ARRAYS = ADDITIVE + TRACK_ROWS
# what a comparison needs equal (the obstacle set is part of what was measured)
OPTION_KEYS = ('dt', 'radius', 'hit_radius', 'r_bin', 'r_bins', 'tau_bin', 'tau_bins', 'box', 'n_obstacles', 'obstacles_hash')


def check_options(dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.05, r_bins=100, tau_bin=0.1, tau_bins=100, box=None,
                  frames=None, T=None, N=None, O=None):
    """ValueError on a bad option; returns (box as 4 floats or None, frames (a, b) or None)."""
    from .ops_metrics import OBS_MAX_BINS, OBS_MAX_N, OBS_MAX_O
    for name, x in (('dt', dt), ('radius', radius), ('hit_radius', hit_radius), ('r_bin', r_bin), ('tau_bin', tau_bin)):
        _positive(name, x)
    _count('r_bins', r_bins, OBS_MAX_BINS)
    _count('tau_bins', tau_bins, OBS_MAX_BINS)
    if box is not None:
        box = tuple(float(v) for v in box)
        if len(box) != 4 or not all(math.isfinite(v) for v in box):
            raise ValueError(f'box must be four finite numbers (x0, x1, y0, y1), got {box}')
        if not (_f32(box[0]) < _f32(box[1]) and _f32(box[2]) < _f32(box[3])):
            raise ValueError(f'box {box} is empty (need x0 < x1 and y0 < y1)')
    frames = _window(frames, T)
    if O is not None and O > OBS_MAX_O:
        raise ValueError(f'obstacle_stats: {O} obstacle points (at most {OBS_MAX_O})')
    if N is not None:
        if N > OBS_MAX_N:
            raise ValueError(f'obstacle_stats: {N} slots per frame (at most {OBS_MAX_N})')
        span = (frames[1] - frames[0]) if frames is not None else (T or 0)
        top = max(1449.0, _f32(_f32(r_bin) * int(r_bins)))
        if not top * Q * N * span < 2.0 ** 63:
            raise ValueError(f'obstacle_stats: {N} slots x {span} frames could overflow the 64-bit sums (speeds below 1449, '
                             f'r_bin * r_bins {r_bin * r_bins})')
    return box, frames


def _obstacle_array(obstacles):
    """(O, 2) float32 contiguous numpy of an obstacle set (tensor, array or list; None or empty -> (0, 2))"""
    if obstacles is None:
        return np.zeros((0, 2), np.float32)
    if isinstance(obstacles, torch.Tensor):
        obstacles = obstacles.detach().cpu().numpy()
    obs = np.ascontiguousarray(np.asarray(obstacles, np.float32).reshape(-1, 2))
    return obs


def obstacles_hash(obstacles):
    """sha256 of the float32 bytes of the (O, 2) obstacle set, hex"""
    return hashlib.sha256(_obstacle_array(obstacles).tobytes()).hexdigest()


def obstacle_spacing(obstacles, chunk=1024):
    """The median distance from a valid obstacle point (both coordinates finite) to its nearest other valid point, float64
    on the host; NaN with fewer than two valid points.  A crossing can pass unseen between two points further apart than
    2 hit_radius.  (GC: 0.05 m.)"""
    obs = _obstacle_array(obstacles).astype(np.float64)
    obs = obs[np.isfinite(obs).all(1)]
    n = obs.shape[0]
    if n < 2:
        return float('nan')
    nearest = np.empty(n)
    for lo in range(0, n, chunk):
        d = obs[lo:lo + chunk, None, :] - obs[None, :, :]
        d2 = (d * d).sum(-1)
        d2[np.arange(d2.shape[0]), np.arange(lo, lo + d2.shape[0])] = np.inf
        nearest[lo:lo + chunk] = np.sqrt(d2.min(1))
    return float(np.median(nearest))


_spacing_of = {}                  # obstacles_hash -> obstacle_spacing
_warned = False


def _warn_sparse(obs, digest, hit_radius):
    """once per process: hit_radius below half the obstacle spacing"""
    global _warned
    if _warned or obs.shape[0] < 2:
        return
    if digest not in _spacing_of:
        _spacing_of[digest] = obstacle_spacing(obs)
    gap = _spacing_of[digest]
    if math.isfinite(gap) and _f32(hit_radius) < 0.5 * gap:
        _warned = True
        warnings.warn(f'obstacle_stats: hit_radius {hit_radius:g} is below half the obstacle spacing {gap:g}: a crossing can '
                      'pass between two obstacle points unseen', stacklevel=3)


def track_histograms(rows, r_bin=0.05, r_bins=100):
    """The host half: trk_min_hist (S, r_bins + 1) and tracks, tracks_hit, tracks_contact (S) int64 from the four (S, N) int64
    track rows (module docstring); r_bin is rounded to float32 first, as the device's option is."""
    fr, co, hi, mn = (np.asarray(rows[k], np.int64) for k in TRACK_ROWS)
    S = fr.shape[0]
    r_bin, r_bins = _f32(r_bin), int(r_bins)
    out = dict(trk_min_hist=np.zeros((S, r_bins + 1), np.int64), tracks=np.zeros(S, np.int64),
               tracks_hit=np.zeros(S, np.int64), tracks_contact=np.zeros(S, np.int64))
    for s in range(S):
        has = fr[s] > 0
        r = mn[s][has].astype(np.float64) / float(Q)
        np.add.at(out['trk_min_hist'][s], np.minimum(np.floor(r / r_bin), r_bins).astype(np.int64), 1)
        out['tracks'][s] = int(has.sum())
        out['tracks_hit'][s] = int((has & (hi[s] > 0)).sum())
        out['tracks_contact'][s] = int((has & (co[s] > 0)).sum())
    return out


class ObstacleStats:
    """The obstacle statistics of S members (numpy int64): focal, steps, contact, hit, clear_sum (S); clear, clear_speed, swept
    (S, r_bins + 1); min_ttc (S, tau_bins + 1); trk_min_hist (S, r_bins + 1) and tracks, tracks_hit, tracks_contact (S) made on
    the host from the track rows trk_frames, trk_contacts, trk_hits, trk_min (S, N), which are kept as they come from the
    device (None once statistics are pooled or merged: tracks of different members do not add).  options: dt, radius,
    hit_radius, r_bin, r_bins, tau_bin, tau_bins, box, n_obstacles, obstacles_hash (sha256 of the obstacle set's float32
    bytes) and frames (None once statistics of different windows are merged).  The derived quantities are those of the
    statistics pooled over the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.int64))
        self.options = dict(options)

    @property
    def members(self):
        return self.focal.shape[0]

    @property
    def r_width(self):
        return float(np.float32(self.options['r_bin']))

    @property
    def tau_width(self):
        return float(np.float32(self.options['tau_bin']))

    @property
    def r_centres(self):
        return (np.arange(self.options['r_bins'], dtype=np.float64) + 0.5) * self.r_width

    @property
    def tau_centres(self):
        return (np.arange(self.options['tau_bins'], dtype=np.float64) + 0.5) * self.tau_width

    def member(self, m):
        """Member m as a one-member ObstacleStats (views)."""
        pick = lambda x: None if x is None else x[m:m + 1]
        return ObstacleStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        pick = lambda x: None if x is None else x[idx]
        return ObstacleStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members, added in member order: a one-member ObstacleStats without track rows."""
        return ObstacleStats({k: _total(getattr(self, k)) for k in ADDITIVE}, self.options)

    @staticmethod
    def merge(stats):
        """Several ObstacleStats with the same options (frames aside) as one member: each pooled, added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def clearance_density(self):
        """(r_bins,) focal agent-frames per focal agent-frame with a clearance and per metre (the rest: beyond the range)"""
        c = self.pooled().clear[0]
        return _nan_div(c[:-1], float(c.sum()) * self.r_width)

    def speed_by_clearance(self, min_count=50):
        """(r_bins + 1,) the mean speed clear_speed / (Q clear) of the focal agent-frames per clearance bin, m/s (the last
        bin is open); NaN where a bin holds fewer than min_count items"""
        p = self.pooled()
        n = p.clear[0]
        ok = (n >= min_count) & (n > 0)
        return np.where(ok, p.clear_speed[0] / (float(Q) * np.where(ok, n, 1)), np.nan)

    def contact_rate(self):
        """contacts per focal agent-frame"""
        p = self.pooled()
        return float(_nan_div(p.contact[0], p.focal[0]))

    def hit_rate(self):
        """hits per step"""
        p = self.pooled()
        return float(_nan_div(p.hit[0], p.steps[0]))

    def hit_track_fraction(self):
        """the share of the tracks with a focal frame that hit an obstacle at least once"""
        p = self.pooled()
        return float(_nan_div(p.tracks_hit[0], p.tracks[0]))

    def contact_track_fraction(self):
        """the share of the tracks with a focal frame that were in contact at least once"""
        p = self.pooled()
        return float(_nan_div(p.tracks_contact[0], p.tracks[0]))

    def min_ttc_density(self):
        """(tau_bins,) smallest time to an obstacle per focal agent-frame with a clearance and per second (the rest: on no
        collision course, or beyond the range)"""
        c = self.pooled().min_ttc[0]
        return _nan_div(c[:-1], float(c.sum()) * self.tau_width)

    def track_min_clearance_density(self):
        """(r_bins,) tracks per track with a focal frame and per metre of their smallest clearance"""
        c = self.pooled().trk_min_hist[0]
        return _nan_div(c[:-1], float(c.sum()) * self.r_width)

    def mean_clearance(self):
        """clear_sum / (Q items) over the items below r_bin * r_bins, metres"""
        p = self.pooled()
        return float(_nan_div(p.clear_sum[0], float(Q) * float(p.clear[0, :-1].sum())))

    def summary(self, min_count=50):
        p = self.pooled()
        return {'r_centres': self.r_centres.tolist(), 'tau_centres': self.tau_centres.tolist(),
                'clearance_density': _json_floats(self.clearance_density()),
                'speed_by_clearance': _json_floats(self.speed_by_clearance(min_count)),
                'min_ttc_density': _json_floats(self.min_ttc_density()),
                'track_min_clearance_density': _json_floats(self.track_min_clearance_density()),
                'mean_clearance': _json_float(self.mean_clearance()), 'contact_rate': _json_float(self.contact_rate()),
                'hit_rate': _json_float(self.hit_rate()), 'hit_track_fraction': _json_float(self.hit_track_fraction()),
                'contact_track_fraction': _json_float(self.contact_track_fraction()),
                'focal': int(p.focal[0]), 'steps': int(p.steps[0]), 'contacts': int(p.contact[0]), 'hits': int(p.hit[0]),
                'tracks': int(p.tracks[0]), 'tracks_hit': int(p.tracks_hit[0]), 'tracks_contact': int(p.tracks_contact[0])}

    def to_json(self, path=None, min_count=50):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION,
             'options': {**o, 'box': None if o.get('box') is None else list(o['box']),
                         'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary(min_count)}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """An ObstacleStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'obstacle stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['box'] = None if o.get('box') is None else tuple(o['box'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several ObstacleStats with the same options (frames aside; the obstacle set included) as one member: each pooled,
    added in list order; no track rows."""
    if not stats:
        raise ValueError('merge: no statistics')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in OPTION_KEYS):
            raise ValueError('merge: the statistics were taken with different options or obstacle sets')
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
    return ObstacleStats(arrays, opts)


def obstacle_stats(P, V, M, obstacles, dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.05, r_bins=100, tau_bin=0.1,
                   tau_bins=100, box=None, frames=None, n_active=None):
    """The obstacle statistics of positions P (S, T, N, 2), velocities V (S, T, N, 2) and presence M (S, T, N) -- (T, N, .)
    is one member -- against the obstacle points `obstacles` (O, 2) in one device call for all members: ObstacleStats.  dt
    the seconds per frame; box (x0, x1, y0, y1) restricts the focal agents; frames (a, b) the window; n_active (S) ints:
    member s's slots at or past n_active[s] never held an agent and are not swept.  Warns once when hit_radius is below half
    of obstacle_spacing(obstacles)."""
    from . import ops_metrics
    P, V, M = _promote(P, V, M)
    S, T, N = P.shape[:3]
    obs = _obstacle_array(obstacles)
    box, frames = check_options(dt, radius, hit_radius, r_bin, r_bins, tau_bin, tau_bins, box, frames, T, N, obs.shape[0])
    frames = frames or (0, T)
    digest = obstacles_hash(obs)
    _warn_sparse(obs, digest, hit_radius)
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.obstacle_stats_frames(P, V, M, torch.from_numpy(obs).to(P.device), dt, radius, hit_radius, r_bin,
                                            int(r_bins), tau_bin, int(tau_bins), box, frames, n_active)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host.update(track_histograms(host, r_bin, int(r_bins)))
    opts = dict(dt=float(dt), radius=float(radius), hit_radius=float(hit_radius), r_bin=float(r_bin), r_bins=int(r_bins),
                tau_bin=float(tau_bin), tau_bins=int(tau_bins), box=box, frames=frames, n_obstacles=int(obs.shape[0]),
                obstacles_hash=digest)
    return ObstacleStats(host, opts)


def obstacle_stats_of_raw(raw_data, obstacles=None, **kw):
    """obstacle_stats of a loaded clip (piml_amd.data.data.RawData: position, velocity, mask_p, obstacles), one member,
    against the clip's own obstacles unless `obstacles` gives another set; dt is the clip's time_unit unless given."""
    kw.setdefault('dt', float(raw_data.time_unit))
    return obstacle_stats(raw_data.position, raw_data.velocity, raw_data.mask_p,
                          raw_data.obstacles if obstacles is None else obstacles, **kw)


def _shares(h):
    return _nan_div(h, np.full(h.shape, float(h.sum())))


def compare_obstacle_stats(a, b, min_count=50):
    """Distances between two ObstacleStats, each pooled over its members:
      clearance_l1, min_ttc_l1, track_min_clearance_l1 = sum |share_a - share_b| over the bins of clear, min_ttc and
          trk_min_hist, the open last bin included (0 .. 2): the L1 distance of the densities times the bin width, plus the
          difference of what lies beyond the range;
      contact_rate_diff, hit_rate_diff, hit_track_fraction_diff, contact_track_fraction_diff, mean_clearance_diff = a's
          minus b's;
      speed_max_diff = max |speed_a - speed_b| of speed_by_clearance over the bins valid in both (NaN when none; speed_bins
          says how many).
    ValueError when the two were taken with different options (dt, the radii, any bin set, the box) or against different
    obstacle sets (their number or the float32 bytes: n_obstacles, obstacles_hash)."""
    for k in OPTION_KEYS:
        if a.options[k] != b.options[k]:
            what = 'obstacle sets' if k in ('n_obstacles', 'obstacles_hash') else 'options'
            raise ValueError(f'compare_obstacle_stats: the {what} differ ({k}: {a.options[k]} vs {b.options[k]})')
    pa, pb = a.pooled(), b.pooled()
    sa, sb = a.speed_by_clearance(min_count), b.speed_by_clearance(min_count)
    both = np.isfinite(sa) & np.isfinite(sb)
    return {'clearance_l1': _l1(_shares(pa.clear[0]), _shares(pb.clear[0])),
            'min_ttc_l1': _l1(_shares(pa.min_ttc[0]), _shares(pb.min_ttc[0])),
            'track_min_clearance_l1': _l1(_shares(pa.trk_min_hist[0]), _shares(pb.trk_min_hist[0])),
            'contact_rate_diff': a.contact_rate() - b.contact_rate(), 'hit_rate_diff': a.hit_rate() - b.hit_rate(),
            'hit_track_fraction_diff': a.hit_track_fraction() - b.hit_track_fraction(),
            'contact_track_fraction_diff': a.contact_track_fraction() - b.contact_track_fraction(),
            'mean_clearance_diff': a.mean_clearance() - b.mean_clearance(),
            'speed_max_diff': float(np.abs(sa - sb)[both].max()) if both.any() else float('nan'),
            'speed_bins': int(both.sum())}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='obstacle statistics (wall clearance, contacts, crossings, time to wall) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--obstacles', type=str, default=None,
                   help='take the obstacle set from this clip for every --data and --ref clip (for simulated clips saved '
                        "without one); default: each clip's own")
    p.add_argument('--box', type=str, default=None,
                   help="x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data, in 0.5 m cells)")
    p.add_argument('--dt', type=float, default=None, help="seconds per frame (default: each clip's time_unit)")
    p.add_argument('--radius', type=float, default=0.25)
    p.add_argument('--hit_radius', type=float, default=0.1)
    p.add_argument('--r_bin', type=float, default=0.05)
    p.add_argument('--r_bins', type=int, default=100)
    p.add_argument('--tau_bin', type=float, default=0.1)
    p.add_argument('--tau_bins', type=int, default=100)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(0.08 if args.dt is None else args.dt, args.radius, args.hit_radius, args.r_bin, args.r_bins,
                      args.tau_bin, args.tau_bins, None if args.box in (None, 'auto') else args.box, args.frames)
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_obstacle_stats(stats, tag, min_count=50, file=sys.stdout):
    p = stats.pooled()
    speed, r = stats.speed_by_clearance(min_count), stats.r_centres
    print(f'[obstaclestats] {tag}: mean speed by clearance (bins with >= {min_count} agent-frames; every bin up to 0.5 m, '
          f'then every tenth)', file=file)
    for k in np.nonzero(np.isfinite(speed[:-1]))[0]:
        if r[k] <= 0.5 or k % 10 == 0:
            print(f'  r {r[k]:6.3f} m: {int(p.clear[0, k]):9d} agent-frames, speed {speed[k]:.4f} m/s', file=file)
    print(f'[obstaclestats] {tag}: {int(p.focal[0])} focal agent-frames against {stats.options["n_obstacles"]} obstacle '
          f'points, mean clearance {stats.mean_clearance():.4f} m, contact rate {stats.contact_rate():.4g} '
          f'({int(p.contact[0])} contacts), hit rate {stats.hit_rate():.4g} ({int(p.hit[0])} hits over {int(p.steps[0])} '
          f'steps); tracks {int(p.tracks[0])}: {stats.hit_track_fraction():.4f} hit, '
          f'{stats.contact_track_fraction():.4f} in contact', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    obstacles = _load(args.obstacles).obstacles if args.obstacles else None
    box = args.box
    if box == 'auto':
        src = ref if ref is not None else raws[0]
        box = auto_box(src.position.numpy(), src.mask_p.numpy(), 0.5)
        print(f'[obstaclestats] --box auto: {",".join(f"{v:g}" for v in box)}')
    kw = dict(radius=args.radius, hit_radius=args.hit_radius, r_bin=args.r_bin, r_bins=args.r_bins, tau_bin=args.tau_bin,
              tau_bins=args.tau_bins, box=box, frames=args.frames)
    if args.dt is not None:
        kw['dt'] = args.dt
    data = merge([obstacle_stats_of_raw(r, obstacles, **kw) for r in raws])
    print_obstacle_stats(data, 'data', args.min_count)
    out = {'data': data.to_json(min_count=args.min_count)}
    if ref is not None:
        rs = obstacle_stats_of_raw(ref, obstacles, **kw)
        print_obstacle_stats(rs, 'ref', args.min_count)
        cmp = compare_obstacle_stats(data, rs, args.min_count)
        print('[obstaclestats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                         for k, v in cmp.items()))
        out['ref'] = rs.to_json(min_count=args.min_count)
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[obstaclestats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
