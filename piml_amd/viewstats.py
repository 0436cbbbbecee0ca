"""Heading-frame pair statistics of crowds: who is where in a walking agent's own view.  The pair, flow and
track statistics are isotropic or follow one agent; these are taken in the frame of the focal agent's heading, where an
anisotropic law shows: the pair distribution over (distance ahead, distance to the left), normalised like Karamouzas,
Skinner and Guy's g(tau) (Phys. Rev. Lett. 113, 238701, 2014) by time-scrambled pairs (agent i at frame t, agent j at frame
t + L) and split by the other agent's direction (standing, with, against, across); the cell of the nearest neighbour; and
the front gap with the speed walked at that gap, the distance-headway / speed relation of Seyfried, Steffen, Klingsch and
Boltes (J. Stat. Mech. P10002, 2005).  The O(N^2) sweeps run in one HIP call for all members and lags
(ops_metrics.view_stats_frames, piml_view_stats).

    python -m piml_amd.viewstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--box x0,x1,y0,y1 | --box auto]
                                 [--lags 64,128,192] [--frames a:b] [--cell 0.25] [--half 12] [--out views.json]

Definitions.  Agent i takes part in slice (member s, frame t) when its mask is 1, both coordinates of its position are
finite and both components of its velocity are below 1024 in magnitude (slots at or past n_active[s] are not swept).  A
mover has sp = sqrt(vx^2 + vy^2) >= v_min and the heading h = v / sp.  It is focal when it takes part, moves and lies in the
box [x0, x1) x [y0, y1) (every participant mover without a box).  Lags (L_1 .. L_K), K <= 8, positive and ascending; lag index
0 is L = 0.  Pair slice (s, t, k), frames[0] <= t and t + L_k < frames[1], pairs every focal i of frame t with every
participant j != i (as a slot) of frame t + L_k, mover or not; pairs are ordered.  Per pair, in float32: d = p_j - p_i,
r = sqrt(|d|^2), pairs at or beyond r_max skipped entirely; a = d.h the distance ahead, l = dy hx - dx hy the distance to the
left; class 0 when j does not move, otherwise with q = h_i.h_j: 1 (with) if q >= cos_same, 2 (against) if q <= -cos_same, 3
(across) else; cell (floor((a + X) / cell), floor((l + X) / cell)) with X = cell * half, counted when it lies in the G x G map,
G = 2 half.  Counts per member and lag index: focal agent-frames, pairs evaluated, map[class, cy, cx]; at lag 0 only, per
focal agent: the cell of its nearest participant (smallest r, ties to the lowest slot; the last bin: outside the map, or
nobody) and, over the participants with a > 0 and |l| < corridor, the smallest a as floor(a / gap_bin) (the last bin: at or
beyond gap_bins * gap_bin, or nobody in front) with the agent's own speed added, in 2^-20 fixed point, to the bin's sum.

Derived quantities (float64, of the statistics pooled over members): the map density of lag k = counts / (pairs of lag k x
cell^2); the scrambled density pools lags 1..K; g_map = lag-0 density / scrambled density where both cells hold at least
min_count pairs; the front/back ratio compares the scrambled-normalised counts ahead and behind within a radius; the
passing side is (L - R) / (L + R) of the oncoming pairs ahead, next to the same number of the scrambled pairs (the chance
level); the headway fit is the count-weighted least-squares line gap = m + s speed through the mean speed per gap bin."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _f32, _json_float, _json_floats, _load, _nan_div, _positive, _promote, _total,
                         _window, auto_box, member_indices, parse_box, parse_frames)
from .pairstats import parse_lags

JSON_VERSION = 1
ARRAYS = ('focal', 'pairs', 'map', 'nn_map', 'front_gap', 'front_speed')
CLASSES = ('standing', 'with', 'against', 'across')
Q = 1 << 20
COS_SAME = float(np.float32(np.cos(np.pi / 4)))
OPTION_KEYS = ('lags', 'v_min', 'cell', 'half', 'cos_same', 'r_max', 'corridor', 'gap_bin', 'gap_bins', 'box')


def check_options(lags=(64, 128, 192), v_min=0.1, cell=0.25, half=12, cos_same=COS_SAME, r_max=None, corridor=0.4,
                  gap_bin=0.1, gap_bins=60, box=None, frames=None, T=None):
    """ValueError on a bad option; returns (lags as a tuple of ints, box as 4 floats or None, frames (a, b) or None)."""
    from .ops_metrics import VIEW_MAX_BINS, VIEW_MAX_HALF, VIEW_MAX_LAGS
    _positive('v_min', v_min)
    _positive('cell', cell)
    _positive('corridor', corridor)
    _positive('gap_bin', gap_bin)
    if isinstance(half, bool) or int(half) != half or not 1 <= int(half) <= VIEW_MAX_HALF:
        raise ValueError(f'half must be an integer in 1..{VIEW_MAX_HALF}, got {half}')
    if isinstance(gap_bins, bool) or int(gap_bins) != gap_bins or not 1 <= int(gap_bins) <= VIEW_MAX_BINS:
        raise ValueError(f'gap_bins must be an integer in 1..{VIEW_MAX_BINS}, got {gap_bins}')
    if isinstance(cos_same, bool) or not (math.isfinite(float(cos_same)) and 0.0 <= _f32(cos_same) <= 1.0):
        raise ValueError(f'cos_same must lie in [0, 1], got {cos_same}')
    if r_max is not None:
        _positive('r_max', r_max)
    lags = tuple(lags)
    if len(lags) > VIEW_MAX_LAGS or any(isinstance(x, bool) or int(x) != x or int(x) < 1 for x in lags) \
            or any(int(lags[i]) >= int(lags[i + 1]) for i in range(len(lags) - 1)):
        raise ValueError(f'lags must be at most {VIEW_MAX_LAGS} positive, distinct, ascending frame counts, got {lags}')
    lags = tuple(int(x) for x in lags)
    if box is not None:
        box = tuple(float(v) for v in box)
        if len(box) != 4 or not all(math.isfinite(v) for v in box):
            raise ValueError(f'box must be four finite numbers (x0, x1, y0, y1), got {box}')
        if not (_f32(box[0]) < _f32(box[1]) and _f32(box[2]) < _f32(box[3])):
            raise ValueError(f'box {box} is empty (need x0 < x1 and y0 < y1)')
    return lags, box, _window(frames, T)


class ViewStats:
    """The heading-frame statistics of S members (numpy int64): focal, pairs (S, K+1); map (S, K+1, 4, G, G) by class
    (CLASSES), distance to the left (rows) and distance ahead (columns); nn_map (S, G G + 1); front_gap (S, gap_bins+1);
    front_speed (S, gap_bins).  options: lags, v_min, cell, half, cos_same, r_max, corridor, gap_bin, gap_bins, box, frames
    (None once statistics of different windows are merged).  The derived quantities are those of the statistics pooled
    over the members."""

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
    def G(self):
        return 2 * int(self.options['half'])

    @property
    def cell_width(self):
        return float(np.float32(self.options['cell']))

    @property
    def gap_width(self):
        return float(np.float32(self.options['gap_bin']))

    @property
    def centres(self):
        """(G,) the cell centres along either axis of the map: distance ahead (columns) or to the left (rows)"""
        return (np.arange(self.G, dtype=np.float64) + 0.5 - self.options['half']) * self.cell_width

    @property
    def gap_centres(self):
        return (np.arange(self.options['gap_bins'], dtype=np.float64) + 0.5) * self.gap_width

    def member(self, m):
        """Member m as a one-member ViewStats (views)."""
        return ViewStats({k: getattr(self, k)[m:m + 1] for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        return ViewStats({k: getattr(self, k)[idx] for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members: a one-member ViewStats."""
        return ViewStats({k: _total(getattr(self, k)) for k in ARRAYS}, self.options)

    @staticmethod
    def merge(stats):
        """Several ViewStats with the same options (frames aside) as one member: each pooled, then added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def _counts(self, cls):
        """(K+1, G, G) float64 pooled counts of one class (index or name) or of all"""
        m = self.pooled().map[0].astype(np.float64)
        if cls is None:
            return m.sum(1)
        return m[:, CLASSES.index(cls) if isinstance(cls, str) else int(cls)]

    def map_density(self, k=0, cls=None):
        """(G, G) pairs of lag index k (of one class, or all) per evaluated pair of that lag and per square metre"""
        return _nan_div(self._counts(cls)[k], np.float64(self.pooled().pairs[0, k]) * self.cell_width ** 2)

    def scrambled_map_density(self, cls=None):
        """(G, G) the map density of lags 1..K pooled (NaN without a lag)"""
        return _nan_div(self._counts(cls)[1:].sum(0), np.float64(self.pooled().pairs[0, 1:].sum()) * self.cell_width ** 2)

    def g_map(self, cls=None, min_count=50):
        """(G, G) lag-0 density / scrambled density; NaN where either cell holds fewer than min_count pairs"""
        c = self._counts(cls)
        c0, cs = c[0], c[1:].sum(0)
        ok = (c0 >= min_count) & (cs >= min_count) & (cs > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(ok, self.map_density(0, cls) / np.where(ok, self.scrambled_map_density(cls), 1.0), np.nan)

    def _normalised(self, region, cls=None):
        """(lag-0 pairs of the cells `region` per lag-0 pair) / (the same of the scrambled pairs)"""
        c, p = self._counts(cls), self.pooled().pairs[0].astype(np.float64)
        return float(_nan_div(_nan_div(c[0][region].sum(), p[0]), _nan_div(c[1:].sum(0)[region].sum(), p[1:].sum())))

    def front_back_ratio(self, r=2.0):
        """The scrambled-normalised count of the cells whose centre lies within r of the agent and ahead of it, over that
        of the cells within r and behind it: 1 when agents keep as much room ahead as behind (NaN without a lag)."""
        a, l = np.meshgrid(self.centres, self.centres)
        near = np.hypot(a, l) < r
        return float(_nan_div(self._normalised(near & (a > 0)), self._normalised(near & (a < 0))))

    def passing_side(self, width=1.0):
        """((L - R) / (L + R), the same of the scrambled pairs): L and R the oncoming (class 2) lag-0 pairs in the cells ahead
        whose centre lies to the left / to the right by less than width.  +1: every oncoming agent passes on the left."""
        a, l = np.meshgrid(self.centres, self.centres)
        ahead = (a > 0) & (np.abs(l) < width)
        c = self._counts(2)

        def side(m):
            left, right = m[ahead & (l > 0)].sum(), m[ahead & (l < 0)].sum()
            return float(_nan_div(left - right, left + right))
        return side(c[0]), side(c[1:].sum(0))

    def nn_density(self):
        """(G, G) nearest neighbours per focal agent-frame and per square metre (the rest: outside the map, or nobody)"""
        p = self.pooled()
        return _nan_div(p.nn_map[0, :-1].reshape(self.G, self.G), np.float64(p.focal[0, 0]) * self.cell_width ** 2)

    def gap_density(self):
        """(gap_bins,) front gaps per focal agent-frame and per metre (the rest: beyond the range, or nobody in front)"""
        p = self.pooled()
        return _nan_div(p.front_gap[0, :-1], np.float64(p.focal[0, 0]) * self.gap_width)

    def mean_front_gap(self):
        """the mean front gap (bin centres) of the focal agents with somebody in front within the range"""
        n = self.pooled().front_gap[0, :-1].astype(np.float64)
        return float(_nan_div((n * self.gap_centres).sum(), n.sum()))

    def headway_speed(self, min_count=20):
        """(gap_bins,) the mean speed of the focal agents per front-gap bin; NaN below min_count agents"""
        p = self.pooled()
        n = p.front_gap[0, :-1]
        ok = (n >= min_count) & (n > 0)
        return np.where(ok, p.front_speed[0] / (np.float64(Q) * np.where(ok, n, 1)), np.nan)

    def headway_fit(self, min_count=20):
        """(m, s): the count-weighted least-squares line gap = m + s speed through (mean speed, gap centre) of the bins with
        at least min_count agents -- Seyfried et al.'s required length m (metres) and time gap s (seconds).  NaN with fewer
        than two bins or no spread in speed."""
        v = self.headway_speed(min_count)
        use = np.isfinite(v)
        if use.sum() < 2:
            return float('nan'), float('nan')
        w = self.pooled().front_gap[0, :-1][use].astype(np.float64)
        x, y = v[use], self.gap_centres[use]
        xm, ym = (w * x).sum() / w.sum(), (w * y).sum() / w.sum()
        sxx = (w * (x - xm) ** 2).sum()
        if not sxx > 0:
            return float('nan'), float('nan')
        s = (w * (x - xm) * (y - ym)).sum() / sxx
        return float(ym - s * xm), float(s)

    def summary(self, min_count=50):
        side, chance = self.passing_side()
        m, s = self.headway_fit()
        p = self.pooled()
        return {'front_back_ratio': _json_float(self.front_back_ratio()), 'passing_side': _json_float(side),
                'passing_side_chance': _json_float(chance), 'headway_intercept': _json_float(m),
                'headway_slope': _json_float(s), 'mean_front_gap': _json_float(self.mean_front_gap()),
                'gap_centres': self.gap_centres.tolist(), 'headway_speed': _json_floats(self.headway_speed()),
                'g_map': [_json_floats(row) for row in self.g_map(min_count=min_count)],
                'focal': int(p.focal[0, 0]), 'pairs': p.pairs[0].tolist()}

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
        """A ViewStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'view stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['lags'] = tuple(o['lags'])
        o['box'] = None if o.get('box') is None else tuple(o['box'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several ViewStats with the same options (frames aside) as one member: each pooled, added in list order."""
    if not stats:
        raise ValueError('merge: no statistics')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in OPTION_KEYS):
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
    return ViewStats(arrays, opts)


def view_stats(P, V, M, lags=(64, 128, 192), box=None, frames=None, n_active=None, v_min=0.1, cell=0.25, half=12,
               cos_same=COS_SAME, r_max=None, corridor=0.4, gap_bin=0.1, gap_bins=60):
    """The heading-frame statistics of positions P (S, T, N, 2), velocities V (S, T, N, 2) and presence M (S, T, N) --
    (T, N, .) is one member -- in one device call for all members and lags: ViewStats.  box (x0, x1, y0, y1) restricts the
    focal agents; frames (a, b) the window; r_max a distance cut-off; n_active (S) ints: member s's slots at or past
    n_active[s] never held an agent and are not swept."""
    from . import ops_metrics
    P, V, M = _promote(P, V, M)
    S, T, N = P.shape[:3]
    lags, box, frames = check_options(lags, v_min, cell, half, cos_same, r_max, corridor, gap_bin, gap_bins, box, frames, T)
    if N > ops_metrics.VIEW_MAX_N:
        raise ValueError(f'view_stats: {N} slots per frame (at most {ops_metrics.VIEW_MAX_N})')
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.view_stats_frames(P, V, M, lags, v_min, cell, int(half), cos_same, r_max, corridor, gap_bin,
                                        int(gap_bins), box, frames, n_active)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    opts = dict(lags=lags, v_min=float(v_min), cell=float(cell), half=int(half), cos_same=float(cos_same),
                r_max=None if r_max is None else float(r_max), corridor=float(corridor), gap_bin=float(gap_bin),
                gap_bins=int(gap_bins), box=box, frames=frames)
    return ViewStats(host, opts)


def view_stats_of_raw(raw_data, **kw):
    """view_stats of a loaded clip (piml_amd.data.data.RawData: position, velocity, mask_p), one member."""
    return view_stats(raw_data.position, raw_data.velocity, raw_data.mask_p, **kw)


def compare_view_stats(a, b, min_count=50):
    """Distances between two ViewStats, each pooled over its members:
      map_l1 = half the L1 distance between the lag-0 maps, each normalised to sum 1 over classes and cells;
      nn_map_l1, gap_l1 = half the L1 distance between the nearest-neighbour cell / front-gap fractions per focal
          agent-frame, the open last bin included;
      g_map_max_diff = max |g_a - g_b| over the cells valid in both (NaN when none; g_map_cells says how many);
      front_back_diff, passing_side_diff, headway_slope_diff, headway_intercept_diff = a's minus b's.
    ValueError when the two were taken with different options (lags, box and frames aside)."""
    for k in OPTION_KEYS:
        if k not in ('lags', 'box') and a.options[k] != b.options[k]:
            raise ValueError(f'compare_view_stats: the options differ ({k}: {a.options[k]} vs {b.options[k]})')
    pa, pb = a.pooled(), b.pooled()

    def half_l1(x, y):
        return float(0.5 * np.abs(_nan_div(x, np.float64(x.sum())) - _nan_div(y, np.float64(y.sum()))).sum())
    ga, gb = a.g_map(min_count=min_count), b.g_map(min_count=min_count)
    both = np.isfinite(ga) & np.isfinite(gb)
    (ma, sa), (mb, sb) = a.headway_fit(), b.headway_fit()
    return {'map_l1': half_l1(pa.map[0, 0], pb.map[0, 0]), 'nn_map_l1': half_l1(pa.nn_map[0], pb.nn_map[0]),
            'gap_l1': half_l1(pa.front_gap[0], pb.front_gap[0]),
            'front_back_diff': a.front_back_ratio() - b.front_back_ratio(),
            'passing_side_diff': a.passing_side()[0] - b.passing_side()[0],
            'g_map_max_diff': float(np.abs(ga - gb)[both].max()) if both.any() else float('nan'),
            'g_map_cells': int(both.sum()), 'headway_slope_diff': sa - sb, 'headway_intercept_diff': ma - mb}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='heading-frame pair statistics (front/back, passing side, headway) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--box', type=str, default=None,
                   help="x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data, in 0.5 m cells)")
    p.add_argument('--lags', type=str, default='64,128,192', help='scrambling lags in frames')
    p.add_argument('--cell', type=float, default=0.25)
    p.add_argument('--half', type=int, default=12)
    p.add_argument('--v_min', type=float, default=0.1)
    p.add_argument('--r_max', type=float, default=None)
    p.add_argument('--corridor', type=float, default=0.4)
    p.add_argument('--gap_bin', type=float, default=0.1)
    p.add_argument('--gap_bins', type=int, default=60)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.lags = parse_lags(args.lags)
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(args.lags, args.v_min, args.cell, args.half, COS_SAME, args.r_max, args.corridor, args.gap_bin,
                      args.gap_bins, None if args.box in (None, 'auto') else args.box, args.frames)
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_view_stats(stats, tag, file=sys.stdout):
    side, chance = stats.passing_side()
    m, s = stats.headway_fit()
    pool = stats.pooled()
    print(f'[viewstats] {tag}: {int(pool.focal[0, 0])} focal agent-frames, {int(pool.pairs[0, 0])} lag-0 pairs; '
          f'front/back ratio {stats.front_back_ratio():.4f}, passing side {side:+.4f} (chance {chance:+.4f}), '
          f'mean front gap {stats.mean_front_gap():.3f} m, headway fit gap = {m:.3f} m + {s:.3f} s x speed', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    box = args.box
    if box == 'auto':
        src = ref if ref is not None else raws[0]
        box = auto_box(src.position.numpy(), src.mask_p.numpy(), 0.5)
        print(f'[viewstats] --box auto: {",".join(f"{v:g}" for v in box)}')
    kw = dict(lags=args.lags, v_min=args.v_min, cell=args.cell, half=args.half, r_max=args.r_max, corridor=args.corridor,
              gap_bin=args.gap_bin, gap_bins=args.gap_bins, box=box, frames=args.frames)
    data = merge([view_stats_of_raw(r, **kw) for r in raws])
    print_view_stats(data, 'data')
    out = {'data': data.to_json(min_count=args.min_count)}
    if ref is not None:
        rs = view_stats_of_raw(ref, **kw)
        print_view_stats(rs, 'ref')
        cmp = compare_view_stats(data, rs, args.min_count)
        print('[viewstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                     for k, v in cmp.items()))
        out['ref'] = rs.to_json(min_count=args.min_count)
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[viewstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
