"""Collective-motion statistics of crowds: whether a crowd organises like a real one, without pairing a
simulated agent with a recorded one.  Three standard observables of pedestrian dynamics: the velocity-velocity correlation
over distance C(r) (do neighbours walk the same way?), the lane-formation order parameter of Rex and Loewen (Phys. Rev. E
75, 051402, 2007) with the chance level of its band counts (do counter-flows separate into lanes?), and the velocity / flow
field on the cells of piml_amd.crowdstats (where does the flow go?).  The O(N^2) same-frame sweep runs in one HIP call for
all members (ops_metrics.flow_stats_frames, piml_flow_stats).

    python -m piml_amd.flowstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--box x0,x1,y0,y1 | --box auto]
                                 [--axis x|y|auto|DEG|ex,ey] [--frames a:b] [--out flow.json]

Definitions.  Agent i takes part in slice (member s, frame t) when its mask is 1, both coordinates of its position are
finite and both components of its velocity are finite and below 1024 in magnitude (slots at or past n_active[s] are not
swept); it is focal when it takes part and lies in the box [x0, x1) x [y0, y1) (every participant without a box).  A mover
has s = sqrt(vx^2 + vy^2) >= v_min and the heading h = v / s; a lane mover has |v.e| >= v_min along the unit axis e and the
direction sigma = sign(v.e).  Pairs are ordered, of one frame, float32, d = p_j - p_i; Q = 2^20:
  corr_pairs, corr_sum (S, r_bins): focal mover i with mover j != i, r = sqrt(|d|^2) < r_max, bin floor(r / r_bin): the
      pairs and the sum of llrintf((h_i.h_j) Q);
  lane_n, lane_sum, lane_same, lane_opp, dir_plus, dir_minus (S, T'): focal lane mover i counts the lane movers j != i with
      |d.e_perp| < lane_width and |d.e| < lane_length, e_perp = (-e_y, e_x), as n_same (sigma_j == sigma_i) or n_opp; with a
      non-empty band phi_i = ((n_same - n_opp) / (n_same + n_opp))^2; per slice the agents with a band, the sum of
      llrintf(phi_i Q), of n_same and of n_opp, and the focal lane movers by sigma;
  map_n, map_vx, map_vy (S, gy, gx), with a box: focal participants of any speed per cell of crowdstats' grid, and the sums
      of llrintf(vx Q), llrintf(vy Q).
A small band gives phi > 0 by chance: the same-direction fraction lane_same / (lane_same + lane_opp) stands next to the one
a random assignment of the directions would give, (n+^2 + n-^2) / (n+ + n-)^2."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _f32, _json_float, _json_floats, _load, _nan_div, _positive, _promote, _total,
                         _window, auto_box, grid_shape, member_indices, parse_box, parse_frames)

JSON_VERSION = 1
Q = 1 << 20
SERIES = ('lane_n', 'lane_sum', 'lane_same', 'lane_opp', 'dir_plus', 'dir_minus')
MAPS = ('map_n', 'map_vx', 'map_vy')
ARRAYS = ('corr_pairs', 'corr_sum') + SERIES + MAPS + ('slices',)
MAX_SPEED = 1024.0
OPTION_KEYS = ('v_min', 'r_bin', 'r_bins', 'r_max', 'axis', 'lane_width', 'lane_length')     # what a comparison needs equal


def parse_axis(axis):
    """'x' -> (1, 0); 'y' -> (0, 1); a number (or its text): the angle in degrees from +x; a 2-vector (or 'ex,ey'): that
    direction, normalised; 'auto' -> 'auto'.  The unit vector is rounded to float32.  ValueError on anything else."""
    if isinstance(axis, str):
        text = axis.strip().lower()
        if text == 'auto':
            return 'auto'
        if text == 'x':
            return (1.0, 0.0)
        if text == 'y':
            return (0.0, 1.0)
        try:
            vals = [float(v) for v in text.split(',')]
        except ValueError:
            raise ValueError(f"axis must be 'x', 'y', 'auto', an angle in degrees or a 2-vector, got {axis!r}") from None
        axis = vals[0] if len(vals) == 1 else vals
    if isinstance(axis, bool):
        raise ValueError(f'axis: got {axis!r}')
    if isinstance(axis, (int, float, np.integer, np.floating)):
        if not math.isfinite(float(axis)):
            raise ValueError(f'axis: the angle must be finite, got {axis}')
        ang = math.radians(float(axis))
        vec = (math.cos(ang), math.sin(ang))
    else:
        vec = tuple(float(v) for v in np.asarray(axis, np.float64).reshape(-1))
        if len(vec) != 2 or not all(math.isfinite(v) for v in vec):
            raise ValueError(f'axis must be two finite numbers, got {axis!r}')
    n = math.hypot(*vec)
    if not n > 0:
        raise ValueError('axis: the zero vector has no direction')
    return (_f32(vec[0] / n), _f32(vec[1] / n))


def check_options(v_min=0.1, r_bin=0.1, r_bins=60, r_max=None, axis='x', lane_width=0.5, lane_length=5.0, cell=0.5,
                  box=None, frames=None, T=None):
    """ValueError on a bad option; returns (r_max as a float -- r_bin * r_bins when None --, axis as a unit 2-tuple or
    'auto', box as 4 floats or None, (gx, gy) or None, frames (a, b) or None)."""
    from .ops_metrics import FLOW_MAX_BINS
    for name, x in (('v_min', v_min), ('r_bin', r_bin), ('lane_width', lane_width), ('lane_length', lane_length),
                    ('cell', cell)):
        _positive(name, x)
    if isinstance(r_bins, bool) or int(r_bins) != r_bins or not 1 <= int(r_bins) <= FLOW_MAX_BINS:
        raise ValueError(f'r_bins must be an integer in 1..{FLOW_MAX_BINS}, got {r_bins}')
    full = _f32(_f32(r_bin) * int(r_bins))
    if r_max is None:
        r_max = full
    else:
        _positive('r_max', r_max)
        if _f32(r_max) > full:
            raise ValueError(f'r_max {r_max} is beyond the bins (r_bin * r_bins = {full:g})')
        r_max = float(r_max)
    axis = parse_axis(axis)
    grid = None
    if box is not None:
        box = tuple(float(v) for v in box)
        if len(box) != 4 or not all(math.isfinite(v) for v in box):
            raise ValueError(f'box must be four finite numbers (x0, x1, y0, y1), got {box}')
        if not (_f32(box[0]) < _f32(box[1]) and _f32(box[2]) < _f32(box[3])):
            raise ValueError(f'box {box} is empty (need x0 < x1 and y0 < y1)')
        grid = grid_shape(box, cell)
    return r_max, axis, box, grid, _window(frames, T)


def auto_axis(P, V, M, n_active=None, frames=None):
    """The principal eigenvector of sum v v^T over the participants of every member (float64 sums on the inputs' device;
    (T, N, .) is one member), as a float32 unit 2-tuple with e_x > 0, or e_y > 0 where e_x == 0.  Its sign is irrelevant:
    every statistic is symmetric under e -> -e apart from swapping dir_plus and dir_minus.  (1, 0) without any motion."""
    P, V, M = (torch.as_tensor(x) for x in (P, V, M))
    if P.dim() == 3:
        P, V, M = P[None], V[None], M[None]
    S, T, N = M.shape
    a, b = frames if frames is not None else (0, T)
    P, V, M = P[:, a:b], V[:, a:b], M[:, a:b]
    part = (M == 1) & torch.isfinite(P).all(-1) & (V.abs() < MAX_SPEED).all(-1)
    if n_active is not None:
        bound = torch.as_tensor(n_active).reshape(-1).to(M.device)
        part &= torch.arange(N, device=M.device)[None, None, :] < bound[:, None, None]
    v = torch.where(part[..., None], V, torch.zeros_like(V)).to(torch.float64).reshape(-1, 2)
    sxx, sxy, syy = float((v[:, 0] * v[:, 0]).sum()), float((v[:, 0] * v[:, 1]).sum()), float((v[:, 1] * v[:, 1]).sum())
    ang = 0.5 * math.atan2(2.0 * sxy, sxx - syy)          # in (-pi/2, pi/2]: cos >= 0
    ex, ey = _f32(math.cos(ang)), _f32(math.sin(ang))
    if ex == 0.0:
        ey = abs(ey)
    return (ex, ey)


class FlowStats:
    """The collective-motion statistics of S members (numpy int64): corr_pairs, corr_sum (S, r_bins); lane_n, lane_sum,
    lane_same, lane_opp, dir_plus, dir_minus (S, T'); map_n, map_vx, map_vy (S, gy, gx) or None without a box; slices (S)
    the number of (member, frame) slices each row holds.  options: v_min, r_bin, r_bins, r_max, axis (the unit vector in
    use), lane_width, lane_length, cell, box, frames (None once statistics of different windows are merged).  The derived
    quantities are those of the statistics pooled over the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.int64))
        self.options = dict(options)

    @property
    def members(self):
        return self.corr_pairs.shape[0]

    @property
    def r_width(self):
        return float(np.float32(self.options['r_bin']))

    @property
    def r_centres(self):
        return (np.arange(self.options['r_bins'], dtype=np.float64) + 0.5) * self.r_width

    def member(self, m):
        """Member m as a one-member FlowStats (views)."""
        pick = lambda x: None if x is None else x[m:m + 1]
        return FlowStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        pick = lambda x: None if x is None else x[idx]
        return FlowStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options)

    def pooled(self):
        """The sum over members, added in member order (the series frame by frame): a one-member FlowStats."""
        return FlowStats({k: _total(getattr(self, k)) for k in ARRAYS}, self.options)

    @staticmethod
    def merge(stats):
        """Several FlowStats with the same options (frames aside) as one member: each pooled, their frames laid end to end
        in the series, correlation rows and maps added in list order."""
        return merge(stats)

    # -- derived, float64, of the pooled statistics
    def velocity_correlation(self, min_count=50):
        """(r_bins,) C(r) = corr_sum / (Q corr_pairs): the mean h_i.h_j of the pairs of a distance bin; NaN where the bin
        holds fewer than min_count pairs"""
        p = self.pooled()
        n = p.corr_pairs[0]
        ok = (n >= min_count) & (n > 0)
        return np.where(ok, p.corr_sum[0] / (float(Q) * np.where(ok, n, 1)), np.nan)

    def correlation_length(self, min_count=50):
        """The distance at which C(r) first falls below 1 / e: over the valid bins in order, the first bin centre with
        C < 1 / e, linearly interpolated from the valid bin before it (that centre itself when there is none); NaN when C
        never falls below."""
        c, r = self.velocity_correlation(min_count), self.r_centres
        level, prev = 1.0 / math.e, None
        for k in np.nonzero(np.isfinite(c))[0]:
            if c[k] < level:
                if prev is None:
                    return float(r[k])
                return float(r[prev] + (c[prev] - level) / (c[prev] - c[k]) * (r[k] - r[prev]))
            prev = k
        return float('nan')

    def lane_order(self):
        """(series, mean): the lane order parameter per frame, lane_sum / (Q lane_n) pooled over the members (NaN in a frame
        without a band), and its mean over all agent-frames with a band"""
        p = self.pooled()
        series = _nan_div(p.lane_sum[0], p.lane_n[0].astype(np.float64) * Q)
        return series, float(_nan_div(p.lane_sum.sum(), float(p.lane_n.sum()) * Q))

    def same_direction_fraction(self):
        """the share of band members that walk the focal agent's way: lane_same / (lane_same + lane_opp)"""
        p = self.pooled()
        return float(_nan_div(p.lane_same.sum(), p.lane_same.sum() + p.lane_opp.sum()))

    def chance_same_fraction(self):
        """the share a random assignment of the directions would give: (n+^2 + n-^2) / (n+ + n-)^2 of the focal lane movers"""
        p = self.pooled()
        a, b = float(p.dir_plus.sum()), float(p.dir_minus.sum())
        return float(_nan_div(a * a + b * b, (a + b) * (a + b)))

    def mean_velocity_field(self):
        """(gy, gx, 2) mean velocity of the focal agent-frames of a cell in m/s (NaN in an empty cell); None without a box"""
        if self.map_n is None:
            return None
        p = self.pooled()
        n = p.map_n[0].astype(np.float64) * Q
        return np.stack([_nan_div(p.map_vx[0], n), _nan_div(p.map_vy[0], n)], -1)

    def flow_field(self):
        """(gy, gx, 2) J = rho u in agents per metre and second, rho = map_n / (slices cell^2) as crowdstats' map density:
        sum v / (slices cell^2) per cell; None without a box"""
        if self.map_n is None:
            return None
        p = self.pooled()
        h = float(np.float32(self.options['cell']))
        return np.stack([p.map_vx[0], p.map_vy[0]], -1) / (float(Q) * float(p.slices[0]) * h * h)

    def summary(self, min_count=50):
        series, mean = self.lane_order()
        p = self.pooled()
        same, chance = self.same_direction_fraction(), self.chance_same_fraction()
        return {'r_centres': self.r_centres.tolist(), 'velocity_correlation': _json_floats(self.velocity_correlation(min_count)),
                'correlation_length': _json_float(self.correlation_length(min_count)), 'lane_order': _json_float(mean),
                'lane_order_series': _json_floats(series), 'same_direction_fraction': _json_float(same),
                'chance_same_fraction': _json_float(chance), 'excess_same_fraction': _json_float(same - chance),
                'corr_pairs': int(p.corr_pairs.sum()), 'lane_agents': int(p.lane_n.sum()),
                'dir_plus': int(p.dir_plus.sum()), 'dir_minus': int(p.dir_minus.sum())}

    def to_json(self, path=None, min_count=50):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION,
             'options': {**o, 'axis': list(o['axis']), 'box': None if o.get('box') is None else list(o['box']),
                         'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary(min_count)}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A FlowStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'flow stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['axis'] = tuple(o['axis'])
        o['box'] = None if o.get('box') is None else tuple(o['box'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several FlowStats with the same options (frames aside) as one member: each pooled, their frames laid end to end in
    the series, correlation rows and maps added in list order."""
    if not stats:
        raise ValueError('merge: no statistics')
    keys = OPTION_KEYS + ('cell', 'box')
    for s in stats[1:]:
        if any(s.options[k] != stats[0].options[k] for k in keys):
            raise ValueError('merge: the statistics were taken with different options')
    pools = [s.pooled() for s in stats]
    arrays = {}
    for k in ARRAYS:
        if k in SERIES:
            arrays[k] = np.concatenate([getattr(p, k) for p in pools], 1)
        elif getattr(pools[0], k) is None:
            arrays[k] = None
        else:
            acc = getattr(pools[0], k).copy()
            for p in pools[1:]:
                acc += getattr(p, k)
            arrays[k] = acc
    opts = dict(stats[0].options)
    if any(s.options.get('frames') != opts.get('frames') for s in stats[1:]):
        opts['frames'] = None
    return FlowStats(arrays, opts)


def flow_stats(P, V, M, v_min=0.1, r_bin=0.1, r_bins=60, r_max=None, axis='x', lane_width=0.5, lane_length=5.0, cell=0.5,
               n_active=None, frames=None, box=None):
    """The collective-motion statistics of positions P (S, T, N, 2), velocities V (S, T, N, 2) and presence M (S, T, N) --
    (T, N, .) is one member -- in one device call for all members: FlowStats.  axis: 'x', 'y', an angle in degrees, a
    2-vector, or 'auto' (auto_axis of the inputs, once for all members); box (x0, x1, y0, y1) restricts the focal agents and
    enables the velocity field with cells of `cell` m; frames (a, b) the window; r_max a cut-off below r_bin * r_bins;
    n_active (S) ints: member s's slots at or past n_active[s] never held an agent and are not swept."""
    from . import ops_metrics
    P, V, M = _promote(P, V, M)
    S, T, N = P.shape[:3]
    r_max, axis, box, grid, frames = check_options(v_min, r_bin, r_bins, r_max, axis, lane_width, lane_length, cell, box,
                                                   frames, T)
    if N > ops_metrics.FLOW_MAX_N:
        raise ValueError(f'flow_stats: {N} slots per frame (at most {ops_metrics.FLOW_MAX_N})')
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    if axis == 'auto':
        axis = auto_axis(P, V, M, n_active, frames)
    out = ops_metrics.flow_stats_frames(P, V, M, v_min, r_bin, int(r_bins), r_max, axis, lane_width, lane_length, box, grid,
                                        cell, frames, n_active)
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    host['slices'] = np.full(S, frames[1] - frames[0], np.int64)
    opts = dict(v_min=float(v_min), r_bin=float(r_bin), r_bins=int(r_bins), r_max=float(r_max), axis=axis,
                lane_width=float(lane_width), lane_length=float(lane_length), cell=float(cell), box=box, frames=frames)
    return FlowStats(host, opts)


def flow_stats_of_raw(raw_data, **kw):
    """flow_stats of a loaded clip (piml_amd.data.data.RawData: position, velocity, mask_p), one member."""
    return flow_stats(raw_data.position, raw_data.velocity, raw_data.mask_p, **kw)


def compare_flow_stats(a, b, min_count=50):
    """Distances between two FlowStats, each pooled over its members:
      corr_max_diff = max |C_a(r) - C_b(r)| over the bins valid in both (NaN when none; corr_bins says how many);
      correlation_length_diff, lane_order_diff = a's minus b's (the mean lane order);
      excess_same_fraction_diff = (observed - chance same-direction fraction) of a minus that of b;
      flow_distance = sum |J_a - J_b| / sum max(|J_a|, |J_b|) over the cells (0 .. 2; None when either side has no map or
          the boxes / cells differ; NaN when both fields vanish).
    ValueError when the two were taken with different options (v_min, the bins, r_max, the axis, the band)."""
    for k in OPTION_KEYS:
        if a.options[k] != b.options[k]:
            raise ValueError(f'compare_flow_stats: the options differ ({k}: {a.options[k]} vs {b.options[k]})')
    ca, cb = a.velocity_correlation(min_count), b.velocity_correlation(min_count)
    both = np.isfinite(ca) & np.isfinite(cb)
    flow = None
    if a.map_n is not None and b.map_n is not None and a.options['box'] == b.options['box'] \
            and a.options['cell'] == b.options['cell']:
        ja, jb = a.flow_field(), b.flow_field()
        den = np.maximum(np.linalg.norm(ja, axis=-1), np.linalg.norm(jb, axis=-1)).sum()
        flow = float(np.linalg.norm(ja - jb, axis=-1).sum() / den) if den > 0 else float('nan')
    excess = lambda s: s.same_direction_fraction() - s.chance_same_fraction()
    return {'corr_max_diff': float(np.abs(ca - cb)[both].max()) if both.any() else float('nan'),
            'corr_bins': int(both.sum()),
            'correlation_length_diff': a.correlation_length(min_count) - b.correlation_length(min_count),
            'lane_order_diff': a.lane_order()[1] - b.lane_order()[1],
            'excess_same_fraction_diff': excess(a) - excess(b),
            'flow_distance': flow}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='collective-motion statistics (velocity correlation, lane order, flow field)')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--box', type=str, default=None,
                   help="x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data, in cells)")
    p.add_argument('--axis', type=str, default='x',
                   help="the lane axis: x, y, an angle in degrees, ex,ey or 'auto' (principal axis of the velocities of "
                        '--ref, else of the first --data)')
    p.add_argument('--v_min', type=float, default=0.1)
    p.add_argument('--r_bin', type=float, default=0.1)
    p.add_argument('--r_bins', type=int, default=60)
    p.add_argument('--r_max', type=float, default=None)
    p.add_argument('--lane_width', type=float, default=0.5)
    p.add_argument('--lane_length', type=float, default=5.0)
    p.add_argument('--cell', type=float, default=0.5)
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        args.axis = check_options(args.v_min, args.r_bin, args.r_bins, args.r_max, args.axis, args.lane_width,
                                  args.lane_length, args.cell, None if args.box in (None, 'auto') else args.box,
                                  args.frames)[1]
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_flow_stats(stats, tag, min_count=50, file=sys.stdout):
    c, r = stats.velocity_correlation(min_count), stats.r_centres
    print(f'[flowstats] {tag}: C(r) (bins with >= {min_count} pairs)', file=file)
    for k in np.nonzero(np.isfinite(c))[0]:
        print(f'  r {r[k]:5.2f} m: C {c[k]:+.4f}', file=file)
    same, chance = stats.same_direction_fraction(), stats.chance_same_fraction()
    p = stats.pooled()
    print(f'[flowstats] {tag}: axis ({stats.options["axis"][0]:.4f}, {stats.options["axis"][1]:.4f}), correlation length '
          f'{stats.correlation_length(min_count):.3f} m, lane order {stats.lane_order()[1]:.4f} over {int(p.lane_n.sum())} '
          f'agent-frames, same-direction fraction {same:.4f} (chance {chance:.4f}), {int(p.dir_plus.sum())} + / '
          f'{int(p.dir_minus.sum())} - lane movers', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    src = ref if ref is not None else raws[0]
    box, axis = args.box, args.axis
    if box == 'auto':
        box = auto_box(src.position.numpy(), src.mask_p.numpy(), args.cell)
        print(f'[flowstats] --box auto: {",".join(f"{v:g}" for v in box)}')
    if axis == 'auto':
        axis = auto_axis(src.position, src.velocity, src.mask_p, frames=args.frames)
        print(f'[flowstats] --axis auto: {axis[0]:.6f},{axis[1]:.6f}')
    kw = dict(v_min=args.v_min, r_bin=args.r_bin, r_bins=args.r_bins, r_max=args.r_max, axis=axis,
              lane_width=args.lane_width, lane_length=args.lane_length, cell=args.cell, box=box, frames=args.frames)
    data = merge([flow_stats_of_raw(r, **kw) for r in raws])
    print_flow_stats(data, 'data', args.min_count)
    out = {'data': data.to_json(min_count=args.min_count)}
    if ref is not None:
        rs = flow_stats_of_raw(ref, **kw)
        print_flow_stats(rs, 'ref', args.min_count)
        cmp = compare_flow_stats(data, rs, args.min_count)
        print('[flowstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                     for k, v in cmp.items()))
        out['ref'] = rs.to_json(min_count=args.min_count)
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[flowstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
