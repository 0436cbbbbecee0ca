"""Time-to-collision and pair-distance statistics of crowds: how agents interact, without pairing a simulated
agent with a recorded one.  Karamouzas, Skinner and Guy (Phys. Rev. Lett. 113, 238701, 2014): the time-to-collision
histogram of the pairs present together, divided by that of time-scrambled pairs (agent i at frame t, agent j at frame
t + L), is g(tau), and E(tau) = -ln g(tau) is an interaction energy that follows a power law (about tau^-2) in real crowds.
The nearest-neighbour distance, the pair-distance ratio g(r) and the overlap rate complement it.  The O(N^2) sweeps run in
one HIP call for all members and lags (ops_metrics.pair_stats_frames, piml_pair_stats).

    python -m piml_amd.pairstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--box x0,x1,y0,y1 | --box auto]
                                 [--lags 64,128,192] [--frames a:b] [--out stats.json]

Definitions.  Agent i takes part in slice (member s, frame t) when its mask is 1 and both coordinates of its position and
both components of its velocity are finite (slots at or past n_active[s] are not swept; on a recorded clip the velocity
requirement drops each agent's last frame); it is focal when it takes part and lies in the box [x0, x1) x [y0, y1) (every
participant without a box).  Lags (L_1 .. L_K), K <= 8, positive and ascending; lag index 0 is L = 0.  Pair slice
(s, t, k), frames[0] <= t and t + L_k < frames[1], pairs every focal i of frame t with every participant j != i (as a slot:
one agent for the whole run) of frame t + L_k; pairs are ordered.  Per pair, in float32: d = p_j - p_i, w = v_j - v_i,
c = |d|^2 - R^2, b = d.w, a = |w|^2; distance sqrt(|d|^2), pairs at or beyond r_max skipped entirely; overlap when c < 0;
otherwise a collision course when b < 0 and disc = b^2 - a c >= 0, tau = c / (-b + sqrt(disc)).  Counts per member and lag
index: focal agent-frames, pairs evaluated, overlapping pairs, collision-course pairs by floor(tau / tau_bin) (those below
tau_bins), pairs by floor(distance / r_bin) (below r_bins); at lag 0 only, each focal agent's nearest participant's
distance bin (nn, last bin = none within r_bins * r_bin) and smallest tau bin over its non-overlapping pairs (min_ttc, last
bin = none below tau_bins * tau_bin).

Derived quantities (float64, of the statistics pooled over members): the tau density of lag k = counts / (pairs of lag k x
tau_bin); the scrambled density pools lags 1..K; g(tau) = lag-0 density / scrambled density where both bins hold at least
min_count pairs; E = -ln g; the energy exponent is the least-squares slope of ln E against ln tau (bin centres) over the
bins with a finite E > 0 in tau_range; g(r) likewise on the distance counts; the overlap rate = overlapping lag-0 pairs per
focal agent-frame."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _count, _f32, _json_float, _json_floats, _load, _nan_div, _positive, _promote, _total,
                         _window, auto_box, member_indices, parse_box, parse_frames)

JSON_VERSION = 1
ARRAYS = ('focal', 'pairs', 'overlap', 'ttc', 'dist', 'nn', 'min_ttc')


def check_options(radius=0.5, lags=(64, 128, 192), tau_bin=0.1, tau_bins=100, r_bin=0.05, r_bins=100, r_max=None,
                  box=None, frames=None, T=None):
    """ValueError on a bad option; returns (lags as a tuple of ints, box as 4 floats or None, frames (a, b) or None)."""
    from .ops_metrics import PAIR_MAX_BINS, PAIR_MAX_LAGS
    _positive('radius', radius)
    _positive('tau_bin', tau_bin)
    _positive('r_bin', r_bin)
    _count('tau_bins', tau_bins, PAIR_MAX_BINS)
    _count('r_bins', r_bins, PAIR_MAX_BINS)
    if r_max is not None:
        _positive('r_max', r_max)
    lags = tuple(lags)
    if len(lags) > PAIR_MAX_LAGS or any(isinstance(x, bool) or int(x) != x or int(x) < 1 for x in lags) \
            or any(int(lags[i]) >= int(lags[i + 1]) for i in range(len(lags) - 1)):
        raise ValueError(f'lags must be at most {PAIR_MAX_LAGS} positive, distinct, ascending frame counts, got {lags}')
    lags = tuple(int(x) for x in lags)
    if box is not None:
        box = tuple(float(v) for v in box)
        if len(box) != 4 or not all(math.isfinite(v) for v in box):
            raise ValueError(f'box must be four finite numbers (x0, x1, y0, y1), got {box}')
        if not (_f32(box[0]) < _f32(box[1]) and _f32(box[2]) < _f32(box[3])):
            raise ValueError(f'box {box} is empty (need x0 < x1 and y0 < y1)')
    return lags, box, _window(frames, T)


class PairStats:
    """The pair statistics of S members (numpy int64): focal, pairs, overlap (S, K+1); ttc (S, K+1, tau_bins); dist (S,
    K+1, r_bins); nn (S, r_bins+1); min_ttc (S, tau_bins+1).  options: radius, lags, tau_bin, tau_bins, r_bin, r_bins,
    r_max, box, frames (None once statistics of different windows are merged).  The derived quantities are those of the
    statistics pooled over the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            setattr(self, k, np.asarray(arrays[k], np.int64))
        self.options = dict(options)

    @property
    def members(self):
        return self.focal.shape[0]

    @property
    def lags(self):
        """(0, L_1, .., L_K): the lag of every lag index"""
        return (0,) + tuple(self.options['lags'])

    @property
    def tau_width(self):
        return float(np.float32(self.options['tau_bin']))

    @property
    def r_width(self):
        return float(np.float32(self.options['r_bin']))

    @property
    def tau_centres(self):
        return (np.arange(self.options['tau_bins'], dtype=np.float64) + 0.5) * self.tau_width

    @property
    def r_centres(self):
        return (np.arange(self.options['r_bins'], dtype=np.float64) + 0.5) * self.r_width

    def member(self, m):
        """Member m as a one-member PairStats (views)."""
        return PairStats({k: getattr(self, k)[m:m + 1] for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        return PairStats({k: getattr(self, k)[idx] for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members: a one-member PairStats."""
        return PairStats({k: _total(getattr(self, k)) for k in ARRAYS}, self.options)

    @staticmethod
    def merge(stats):
        """Several PairStats with the same options (frames aside) as one member: each pooled, then added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def _density(self, counts, total, width):
        return _nan_div(counts, np.asarray(total, np.float64) * width)

    def ttc_density(self, k=0):
        """(tau_bins,) collision-course pairs of lag index k per evaluated pair of that lag and per second"""
        p = self.pooled()
        return self._density(p.ttc[0, k], p.pairs[0, k], self.tau_width)

    def scrambled_ttc_density(self):
        """(tau_bins,) the tau density of lags 1..K pooled (NaN without a lag)"""
        p = self.pooled()
        return self._density(p.ttc[0, 1:].sum(0), p.pairs[0, 1:].sum(), self.tau_width)

    def dist_density(self, k=0):
        """(r_bins,) pairs of lag index k per evaluated pair of that lag and per metre"""
        p = self.pooled()
        return self._density(p.dist[0, k], p.pairs[0, k], self.r_width)

    def scrambled_dist_density(self):
        p = self.pooled()
        return self._density(p.dist[0, 1:].sum(0), p.pairs[0, 1:].sum(), self.r_width)

    def _ratio(self, counts, dens0, dens_s, min_count):
        c0, cs = counts[0, 0], counts[0, 1:].sum(0)
        ok = (c0 >= min_count) & (cs >= min_count) & (cs > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(ok, dens0 / np.where(ok, dens_s, 1.0), np.nan)

    def g_tau(self, min_count=50):
        """(tau_bins,) g(tau) = lag-0 tau density / scrambled tau density; NaN where either bin holds < min_count pairs"""
        return self._ratio(self.pooled().ttc, self.ttc_density(0), self.scrambled_ttc_density(), min_count)

    def interaction_energy(self, min_count=50):
        """(tau_bins,) E(tau) = -ln g(tau)"""
        g = self.g_tau(min_count)
        with np.errstate(divide='ignore', invalid='ignore'):
            return -np.log(g)

    def energy_exponent(self, tau_range=(0.2, 2.5), min_count=50):
        """(p, n): the least-squares slope p of ln E against ln tau over the bins whose centre lies in tau_range and whose
        E is finite and > 0 (E ~ tau^p; about -2 in real crowds), and the number n of bins used (p NaN when n < 2)."""
        e = self.interaction_energy(min_count)
        tau = self.tau_centres
        use = np.isfinite(e) & (e > 0) & (tau >= tau_range[0]) & (tau <= tau_range[1])
        n = int(use.sum())
        if n < 2:
            return float('nan'), n
        x, y = np.log(tau[use]), np.log(e[use])
        x0, y0 = x - x.mean(), y - y.mean()
        return float((x0 * y0).sum() / (x0 * x0).sum()), n

    def g_r(self, min_count=50):
        """(r_bins,) g(r) = lag-0 distance density / scrambled distance density, NaN like g_tau"""
        return self._ratio(self.pooled().dist, self.dist_density(0), self.scrambled_dist_density(), min_count)

    def nn_density(self):
        """(r_bins,) nearest-neighbour distances per focal agent-frame and per metre (the rest: none within the range)"""
        p = self.pooled()
        return self._density(p.nn[0, :-1], p.focal[0, 0], self.r_width)

    def min_ttc_density(self):
        """(tau_bins,) smallest tau per focal agent-frame and per second (the rest: none below the range)"""
        p = self.pooled()
        return self._density(p.min_ttc[0, :-1], p.focal[0, 0], self.tau_width)

    def overlap_rate(self):
        """overlapping ordered lag-0 pairs per focal agent-frame"""
        p = self.pooled()
        return float(_nan_div(p.overlap[0, 0], p.focal[0, 0]))

    def summary(self, min_count=50):
        p, n = self.energy_exponent(min_count=min_count)
        return {'tau_centres': self.tau_centres.tolist(), 'g_tau': _json_floats(self.g_tau(min_count)),
                'interaction_energy': _json_floats(self.interaction_energy(min_count)),
                'energy_exponent': _json_float(p), 'energy_bins': n, 'g_r': _json_floats(self.g_r(min_count)),
                'overlap_rate': _json_float(self.overlap_rate()),
                'focal': int(self.pooled().focal[0, 0]), 'pairs': self.pooled().pairs[0].tolist()}

    def to_json(self, path=None, min_count=50):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION,
             'options': {**o, 'lags': list(o['lags']), 'box': None if o.get('box') is None else list(o['box']),
                         'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary(min_count)}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A PairStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'pair stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['lags'] = tuple(o['lags'])
        o['box'] = None if o.get('box') is None else tuple(o['box'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several PairStats with the same options (frames aside) as one member: each pooled, added in list order."""
    if not stats:
        raise ValueError('merge: no statistics')
    keys = ('radius', 'lags', 'tau_bin', 'tau_bins', 'r_bin', 'r_bins', 'r_max', 'box')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in keys):
            raise ValueError('merge: the statistics were taken with different options')
    pools = [s.pooled() for s in stats]
    arrays = {}
    for k in ARRAYS:
        acc = getattr(pools[0], k).copy()
        for p in pools[1:]:
            acc += getattr(p, k)
        arrays[k] = acc
    opts = dict(stats[0].options)
    if any(s.options.get('frames') != opts.get('frames') for s in stats[1:]):
        opts['frames'] = None
    return PairStats(arrays, opts)


def pair_stats(P, V, M, radius=0.5, lags=(64, 128, 192), tau_bin=0.1, tau_bins=100, r_bin=0.05, r_bins=100, r_max=None,
               box=None, frames=None, n_active=None):
    """The pair statistics of positions P (S, T, N, 2), velocities V (S, T, N, 2) and presence M (S, T, N) -- (T, N, .) is
    one member -- in one device call for all members and lags: PairStats.  box (x0, x1, y0, y1) restricts the focal agents;
    frames (a, b) the window; r_max a distance cut-off; n_active (S) ints: member s's slots at or past n_active[s] never
    held an agent and are not swept."""
    from . import ops_metrics
    P, V, M = _promote(P, V, M)
    S, T, N = P.shape[:3]
    lags, box, frames = check_options(radius, lags, tau_bin, tau_bins, r_bin, r_bins, r_max, box, frames, T)
    if N > ops_metrics.PAIR_MAX_N:
        raise ValueError(f'pair_stats: {N} slots per frame (at most {ops_metrics.PAIR_MAX_N})')
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.pair_stats_frames(P, V, M, radius, lags, tau_bin, int(tau_bins), r_bin, int(r_bins), r_max, box,
                                        frames, n_active)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    opts = dict(radius=float(radius), lags=lags, tau_bin=float(tau_bin), tau_bins=int(tau_bins), r_bin=float(r_bin),
                r_bins=int(r_bins), r_max=None if r_max is None else float(r_max), box=box, frames=frames)
    return PairStats(host, opts)


def pair_stats_of_raw(raw_data, **kw):
    """pair_stats of a loaded clip (piml_amd.data.data.RawData: position, velocity, mask_p), one member."""
    return pair_stats(raw_data.position, raw_data.velocity, raw_data.mask_p, **kw)


def compare_pair_stats(a, b, min_count=50):
    """Distances between two PairStats, each pooled over its members:
      ttc_l1 = sum_b |rho_a - rho_b| tau_bin of the lag-0 tau densities;
      nn_l1 = sum |f_a - f_b| of the nearest-neighbour fractions per focal agent-frame, the open last bin included;
      g_tau_max_diff = max |g_a(tau) - g_b(tau)| over the bins valid in both (NaN when none; g_tau_bins says how many);
      energy_exponent_diff, overlap_rate_diff = a's minus b's."""
    for k in ('tau_bin', 'tau_bins', 'r_bin', 'r_bins'):
        if a.options[k] != b.options[k]:
            raise ValueError(f'compare_pair_stats: the bins differ ({k})')
    pa, pb = a.pooled(), b.pooled()
    ttc_l1 = float(np.nansum(np.abs(a.ttc_density(0) - b.ttc_density(0))) * a.tau_width)
    fa, fb = _nan_div(pa.nn[0], pa.focal[0, 0]), _nan_div(pb.nn[0], pb.focal[0, 0])
    nn_l1 = float(np.abs(fa - fb).sum())
    ga, gb = a.g_tau(min_count), b.g_tau(min_count)
    both = np.isfinite(ga) & np.isfinite(gb)
    g_diff = float(np.abs(ga - gb)[both].max()) if both.any() else float('nan')
    return {'ttc_l1': ttc_l1, 'nn_l1': nn_l1, 'g_tau_max_diff': g_diff, 'g_tau_bins': int(both.sum()),
            'energy_exponent_diff': a.energy_exponent(min_count=min_count)[0] - b.energy_exponent(min_count=min_count)[0],
            'overlap_rate_diff': a.overlap_rate() - b.overlap_rate()}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def parse_lags(text):
    """'64,128,192' -> (64, 128, 192); '' -> ()"""
    return tuple(int(v) for v in text.split(',') if v.strip())


def get_args(argv=None):
    p = argparse.ArgumentParser(description='time-to-collision and pair-distance statistics (g(tau), E(tau)) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--box', type=str, default=None,
                   help="x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data, in 0.5 m cells)")
    p.add_argument('--lags', type=str, default='64,128,192', help='scrambling lags in frames')
    p.add_argument('--radius', type=float, default=0.5)
    p.add_argument('--tau_bin', type=float, default=0.1)
    p.add_argument('--tau_bins', type=int, default=100)
    p.add_argument('--r_bin', type=float, default=0.05)
    p.add_argument('--r_bins', type=int, default=100)
    p.add_argument('--r_max', type=float, default=None)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.lags = parse_lags(args.lags)
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(args.radius, args.lags, args.tau_bin, args.tau_bins, args.r_bin, args.r_bins, args.r_max,
                      None if args.box in (None, 'auto') else args.box, args.frames)
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_pair_stats(stats, tag, min_count=50, file=sys.stdout):
    g, e = stats.g_tau(min_count), stats.interaction_energy(min_count)
    tau = stats.tau_centres
    print(f'[pairstats] {tag}: g(tau), E(tau) = -ln g (bins with >= {min_count} pairs at lag 0 and scrambled)', file=file)
    for k in np.nonzero(np.isfinite(g))[0]:
        print(f'  tau {tau[k]:6.2f} s: g {g[k]:.4f}  E {e[k]:+.4f}', file=file)
    p, n = stats.energy_exponent(min_count=min_count)
    pool = stats.pooled()
    print(f'[pairstats] {tag}: {int(pool.focal[0, 0])} focal agent-frames, {int(pool.pairs[0, 0])} lag-0 pairs, '
          f'energy exponent {p:.4f} over {n} bins, overlap rate {stats.overlap_rate():.4g}', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    box = args.box
    if box == 'auto':
        src = ref if ref is not None else raws[0]
        box = auto_box(src.position.numpy(), src.mask_p.numpy(), 0.5)
        print(f'[pairstats] --box auto: {",".join(f"{v:g}" for v in box)}')
    kw = dict(radius=args.radius, lags=args.lags, tau_bin=args.tau_bin, tau_bins=args.tau_bins, r_bin=args.r_bin,
              r_bins=args.r_bins, r_max=args.r_max, box=box, frames=args.frames)
    data = merge([pair_stats_of_raw(r, **kw) for r in raws])
    print_pair_stats(data, 'data', args.min_count)
    out = {'data': data.to_json(min_count=args.min_count)}
    if ref is not None:
        rs = pair_stats_of_raw(ref, **kw)
        print_pair_stats(rs, 'ref', args.min_count)
        cmp = compare_pair_stats(data, rs, args.min_count)
        print('[pairstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                     for k, v in cmp.items()))
        out['ref'] = rs.to_json(min_count=args.min_count)
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[pairstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
