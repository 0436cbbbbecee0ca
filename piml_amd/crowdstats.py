"""Crowd-dynamics statistics that need no agent pairing: the speed-density relation (fundamental
diagram) on a local density per agent -- a Gaussian kernel sum or the Voronoi density of Steffen and Seyfried (2010) --
time-averaged density maps and per-frame occupancy / speed / density series, for simulated scenes, ensembles and recorded
clips.  Everything runs in one HIP call for all members (ops_metrics.crowd_stats_frames, piml_crowd_stats;
ops_metrics.crowd_stats_voronoi_frames, piml_crowd_stats_voronoi).

    python -m piml_amd.crowdstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--box x0,x1,y0,y1 | --box auto]
                                  [--radius 0.7] [--cell 0.5] [--frames a:b] [--out stats.json]
                                  [--density voronoi [--cutoff 1.0] [--bounds x0,x1,y0,y1 | --bounds auto]]

Definitions, for every focal agent i of slice (member s, frame t): present = mask 1 and a finite position; focal = present
and inside the box [x0, x1) x [y0, y1) (every present agent without a box); rho_i = sum_j exp(-|p_j - p_i|^2 / R^2) /
(pi R^2) over the slice's present j, j = i included; u_i = |v_i| where the velocity is finite; bin = min(floor(rho_i /
rho_bin), rho_bins - 1); map cell (floor((x - x0) / h), floor((y - y0) / h)).  With density='voronoi', rho_i = 1 / area of
the agent's Voronoi cell among the slice's present agents, cut off at a regular polygon of `sides` vertices and radius
`cutoff` around it and at the walkable rectangle `bounds` (outside which no agent is focal); agents whose cell cannot be
formed are left out and counted in `dropped` (include/piml_hip.h has the clip rules)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

JSON_VERSION = 1
ARRAYS = ('n', 'n_speed', 'sum_speed', 'sum_density', 'fd_count', 'fd_sum', 'fd_sum2', 'map', 'slices', 'dropped')
DENSITIES = ('gaussian', 'voronoi')
DENSITY_KEYS = ('density', 'cutoff', 'bounds', 'sides')       # the options that say which density the abscissa is
VORONOI_SIDES = 16
VORONOI_MAX_SIDES = 32


def _f32(x):
    return float(np.float32(x))


# What the statistics modules' option checks, entries and comparisons share.
def _positive(name, x):
    if isinstance(x, bool) or not (math.isfinite(float(x)) and float(x) > 0 and _f32(x) > 0 and math.isfinite(_f32(x))):
        raise ValueError(f'{name} must be a positive number, got {x}')


def _count(name, x, hi):
    if isinstance(x, bool) or int(x) != x or not 1 <= int(x) <= hi:
        raise ValueError(f'{name} must be an integer in 1..{hi}, got {x}')


def _window(frames, T):
    """frames as (a, b) ints, or None; ValueError unless 0 <= a < b (<= T when T is known)"""
    if frames is None:
        return None
    a, b = (int(v) for v in frames)
    if a < 0 or b <= a or (T is not None and b > T):
        raise ValueError(f'frames must satisfy 0 <= a < b <= {T}, got {tuple(frames)}')
    return a, b


def _bounds(n_active, S, N, device):
    """n_active as an int32 (S,) tensor on the device, clamped to [0, N]; None stays None"""
    if n_active is None:
        return None
    n_active = torch.as_tensor(n_active).reshape(-1)
    if n_active.numel() != S:
        raise ValueError(f'n_active: {n_active.numel()} bounds for {S} members')
    return n_active.clamp(0, N).to(device=device, dtype=torch.int32)


def _total(x):
    """sum over the member axis, added in member order, keeping it; None stays None"""
    if x is None:
        return None
    acc = x[0].copy()
    for m in range(1, x.shape[0]):
        acc += x[m]
    return acc[None]


def _l1(x, y):
    """sum |x - y| of two share vectors (0 .. 2); NaN when either has no items"""
    return float(np.abs(x - y).sum()) if np.isfinite(x).all() and np.isfinite(y).all() else float('nan')


def grid_shape(box, cell):
    """(gx, gy) = (ceil((x1 - x0) / h), ceil((y1 - y0) / h)) of the float32 box and cell, in float64 on the host."""
    x0, x1, y0, y1 = (_f32(v) for v in box)
    h = _f32(cell)
    return int(math.ceil((x1 - x0) / h)), int(math.ceil((y1 - y0) / h))


def voronoi_dirs(sides=VORONOI_SIDES):
    """(sides, 2) float32: (cos, sin) of 2 pi k / sides, evaluated in float64 and rounded; the cut-off polygon's vertices
    are cutoff * dirs[k] on the host and on the device alike."""
    ang = 2.0 * np.pi * np.arange(int(sides), dtype=np.float64) / int(sides)
    return np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)


def check_density(density='gaussian', cutoff=None, bounds=None, sides=None):
    """ValueError on a bad density option; returns the four as the options record them: ('gaussian', None, None, None) or
    ('voronoi', cutoff (default 1.0), bounds as 4 floats or None, sides (default 16))."""
    if density not in DENSITIES:
        raise ValueError(f'density must be one of {DENSITIES}, got {density!r}')
    if density == 'gaussian':
        if cutoff is not None or bounds is not None or sides is not None:
            raise ValueError("cutoff, bounds and sides belong to density='voronoi'")
        return density, None, None, None
    cutoff = 1.0 if cutoff is None else float(cutoff)
    if not (math.isfinite(cutoff) and _f32(cutoff) > 0 and math.isfinite(_f32(cutoff))):
        raise ValueError(f'cutoff must be a positive number, got {cutoff}')
    sides = VORONOI_SIDES if sides is None else sides
    if isinstance(sides, bool) or int(sides) != sides or not 3 <= int(sides) <= VORONOI_MAX_SIDES:
        raise ValueError(f'sides must be an integer in 3..{VORONOI_MAX_SIDES}, got {sides}')
    if bounds is not None:
        bounds = tuple(float(v) for v in bounds)
        if len(bounds) != 4 or not all(math.isfinite(v) for v in bounds):
            raise ValueError(f'bounds must be four finite numbers (x0, x1, y0, y1), got {bounds}')
        if not (_f32(bounds[0]) < _f32(bounds[1]) and _f32(bounds[2]) < _f32(bounds[3])):
            raise ValueError(f'bounds {bounds} are empty (need x0 < x1 and y0 < y1)')
    return density, cutoff, bounds, int(sides)


def check_options(radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=24, frames=None, T=None, density='gaussian',
                  cutoff=None, bounds=None, sides=None):
    """ValueError on a bad option; returns (box as 4 floats or None, (gx, gy) or None, frames (a, b) or None)."""
    from .ops_metrics import CROWD_MAX_BINS
    check_density(density, cutoff, bounds, sides)
    if not (math.isfinite(float(radius)) and float(radius) > 0):
        raise ValueError(f'radius must be a positive number, got {radius}')
    if not (math.isfinite(float(rho_bin)) and float(rho_bin) > 0):
        raise ValueError(f'rho_bin must be a positive number, got {rho_bin}')
    _count('rho_bins', rho_bins, CROWD_MAX_BINS)
    grid = None
    if box is not None:
        box = tuple(float(v) for v in box)
        if len(box) != 4 or not all(math.isfinite(v) for v in box):
            raise ValueError(f'box must be four finite numbers (x0, x1, y0, y1), got {box}')
        if not (_f32(box[0]) < _f32(box[1]) and _f32(box[2]) < _f32(box[3])):
            raise ValueError(f'box {box} is empty (need x0 < x1 and y0 < y1)')
        if not (math.isfinite(float(cell)) and float(cell) > 0):
            raise ValueError(f'cell must be a positive number, got {cell}')
        grid = grid_shape(box, cell)
    return box, grid, _window(frames, T)


def _promote(P, V, M):
    """(T, N, .) -> (1, T, N, .); torch or numpy in, float32 contiguous on a GPU out."""
    dev = next((x.device for x in (P, V, M) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device('cuda'))
    P, V, M = (torch.as_tensor(x) for x in (P, V, M))
    if P.dim() == 3:
        P, V, M = P[None], V[None], M[None]
    if P.dim() != 4 or P.shape[-1] != 2 or tuple(V.shape) != tuple(P.shape) or tuple(M.shape) != tuple(P.shape[:3]):
        raise ValueError(f'expected P, V (S, T, N, 2) or (T, N, 2) and M (S, T, N) or (T, N), got {tuple(P.shape)}, '
                         f'{tuple(V.shape)}, {tuple(M.shape)}')
    if min(P.shape[:3]) < 1:
        raise ValueError(f'empty input {tuple(P.shape)}')
    return tuple(x.to(device=dev, dtype=torch.float32).contiguous() for x in (P, V, M))


def _nan_div(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(b > 0, a / np.where(b > 0, b, 1), np.nan)


def member_indices(members, count):
    """`members` as an int64 index array into `count` members; IndexError on anything but integers in 0 .. count - 1."""
    idx = list(members)
    for m in idx:
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) < count:
            raise IndexError(f'member {m!r} of {count}')
    return np.asarray(idx, np.int64).reshape(-1)


class CrowdStats:
    """The statistics of S members over T' frames.  Raw arrays (numpy): n, n_speed (S, T') int64 focal agents / those with
    a speed; sum_speed, sum_density (S, T') float64; fd_count (S, B) int64, fd_sum, fd_sum2 (S, B) float64 (count, sum u,
    sum u^2 per density bin); map (S, gy, gx) int64 focal agent-frames per cell (None without a box); density (S, T', N)
    float32 per-agent density (NaN where not focal; None unless asked for); slices (S) the number of (member, frame)
    slices each row holds (T' per member, more once pooled); dropped (S) focal agents left out because their Voronoi cell
    could not be formed (0 for the Gaussian density).  options: radius, box, cell, rho_bin, rho_bins, frames and
    density, cutoff, bounds, sides ('gaussian', None, None, None where they are not given)."""

    def __init__(self, arrays, options, density=None):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.float64 if k in ('sum_speed', 'sum_density', 'fd_sum',
                                                                                    'fd_sum2') else np.int64))
        if self.dropped is None:
            self.dropped = np.zeros(self.n.shape[0], np.int64)
        self.density = density
        self.options = {'density': 'gaussian', 'cutoff': None, 'bounds': None, 'sides': None, **options}

    @property
    def members(self):
        return self.n.shape[0]

    @property
    def bin_edges(self):
        """lower edges of the density bins (m^-2); the last bin is open-ended"""
        return np.arange(self.options['rho_bins'], dtype=np.float64) * np.float32(self.options['rho_bin'])

    @property
    def mean_speed(self):
        """(S, T') mean speed of the focal agents with a speed (NaN in a frame without any)"""
        return _nan_div(self.sum_speed, self.n_speed)

    @property
    def mean_density(self):
        """(S, T') mean local density of the focal agents (NaN in a frame without any)"""
        return _nan_div(self.sum_density, self.n)

    @property
    def fd_mean(self):
        """(S, B) mean speed per density bin (NaN in an empty bin)"""
        return _nan_div(self.fd_sum, self.fd_count)

    @property
    def fd_std(self):
        """(S, B) population standard deviation of the speed per density bin (NaN in an empty bin)"""
        mean = self.fd_mean
        return np.sqrt(np.maximum(_nan_div(self.fd_sum2, self.fd_count) - mean * mean, 0.0))

    @property
    def map_density(self):
        """(S, gy, gx) time-averaged agents per m^2: map / (slices * cell^2); None without a box"""
        if self.map is None:
            return None
        h = float(np.float32(self.options['cell']))
        return self.map / (self.slices[:, None, None].astype(np.float64) * h * h)

    def member(self, m):
        """Member m as a one-member CrowdStats (views)."""
        pick = lambda x: None if x is None else x[m:m + 1]
        return CrowdStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options, density=pick(self.density))

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        pick = lambda x: None if x is None else x[idx]
        return CrowdStats({k: pick(getattr(self, k)) for k in ARRAYS}, self.options, density=pick(self.density))

    def pooled(self):
        """The sum over members, added in member order: a one-member CrowdStats (no per-agent density)."""
        def total(x):
            if x is None:
                return None
            acc = x[0].copy()
            for m in range(1, x.shape[0]):
                acc += x[m]
            return acc[None]
        return CrowdStats({k: total(getattr(self, k)) for k in ARRAYS}, self.options)

    def to_json(self, path=None):
        """A JSON-ready dict of the options, the raw arrays and the derived pooled summary; written to path if given."""
        pool = self.pooled()
        d = {'version': JSON_VERSION, 'options': {**self.options,
                                                 'box': None if self.options.get('box') is None else list(self.options['box']),
                                                 'bounds': None if self.options.get('bounds') is None
                                                 else list(self.options['bounds']),
                                                 'frames': list(self.options['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': {'bin_edges': self.bin_edges.tolist(), 'fd_count': pool.fd_count[0].tolist(),
                        'fd_mean': _json_floats(pool.fd_mean[0]), 'fd_std': _json_floats(pool.fd_std[0]),
                        'mean_speed': _json_float(_nan_div(pool.sum_speed.sum(), pool.n_speed.sum())),
                        'mean_density': _json_float(_nan_div(pool.sum_density.sum(), pool.n.sum()))}}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A CrowdStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'crowd stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        opts = dict(src['options'])
        opts['box'] = None if opts.get('box') is None else tuple(opts['box'])
        opts['bounds'] = None if opts.get('bounds') is None else tuple(opts['bounds'])
        opts['frames'] = tuple(opts['frames'])
        return cls(src['arrays'], opts)


def _json_float(x):
    x = float(x)
    return x if math.isfinite(x) else None


def _json_floats(a):
    return [_json_float(x) for x in np.asarray(a).ravel()]


def crowd_stats(P, V, M, radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=24, frames=None, return_density=False,
                n_active=None, density='gaussian', cutoff=None, bounds=None, sides=None):
    """The statistics of positions P (S, T, N, 2), velocities V (S, T, N, 2) and presence M (S, T, N) -- (T, N, .) is one
    member -- in one device call for all members: CrowdStats.  box (x0, x1, y0, y1) restricts the focal agents and enables
    the map with cells of `cell` m; frames (a, b) a frame range; n_active (S) ints: member s's slots at or past
    n_active[s] never held an agent and are not swept.  density 'gaussian' (radius) or 'voronoi' (radius is ignored;
    cutoff, default 1.0 m; bounds (x0, x1, y0, y1), the walkable rectangle, or None; sides of the cut-off polygon, default
    16): cutoff, bounds and sides are an error with 'gaussian'."""
    from . import ops_metrics
    P, V, M = _promote(P, V, M)
    S, T, N = P.shape[:3]
    box, grid, frames = check_options(radius, box, cell, rho_bin, rho_bins, frames, T)
    density, cutoff, bounds, sides = check_density(density, cutoff, bounds, sides)
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    if density == 'voronoi':
        out = ops_metrics.crowd_stats_voronoi_frames(P, V, M, cutoff, voronoi_dirs(sides), bounds, box, grid, cell, rho_bin,
                                                     int(rho_bins), frames, return_density, n_active)
    else:
        out = ops_metrics.crowd_stats_frames(P, V, M, radius, box, grid, cell, rho_bin, int(rho_bins), frames,
                                             return_density, n_active)
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    host['slices'] = np.full(S, frames[1] - frames[0], np.int64)
    opts = dict(radius=float(radius), box=box, cell=float(cell), rho_bin=float(rho_bin), rho_bins=int(rho_bins),
                frames=frames, density=density, cutoff=cutoff, bounds=bounds, sides=sides)
    return CrowdStats(host, opts, density=host.pop('density'))


def crowd_stats_of_raw(raw_data, **kw):
    """crowd_stats of a loaded clip (piml_amd.data.data.RawData: position, velocity, mask_p), one member."""
    return crowd_stats(raw_data.position, raw_data.velocity, raw_data.mask_p, **kw)


def call_options(stats):
    """The keywords that make crowd_stats take statistics comparable with `stats` (its options, frames aside)."""
    keys = ('radius', 'box', 'cell', 'rho_bin', 'rho_bins')
    if stats.options['density'] != 'gaussian':
        keys += DENSITY_KEYS
    return {k: stats.options[k] for k in keys}


def same_density(a, b):
    """Whether two CrowdStats measure density the same way: kind, cut-off, bounds and sides (and, for the Gaussian kind,
    nothing else: different radii were comparable before there was a second kind and stay so)."""
    return all(a.options[k] == b.options[k] for k in DENSITY_KEYS)


def merge(stats):
    """Several CrowdStats with the same options (frames aside) as one member: each pooled, their frames laid end to end
    in the series, diagrams and maps added in list order."""
    if not stats:
        raise ValueError('merge: no statistics')
    pools = [s.pooled() for s in stats]
    keys = ('radius', 'box', 'cell', 'rho_bin', 'rho_bins') + DENSITY_KEYS
    for p in pools[1:]:
        if any(p.options[k] != pools[0].options[k] for k in keys):
            raise ValueError('merge: the statistics were taken with different options')
    arrays = {}
    for k in ARRAYS:
        if k in ('n', 'n_speed', 'sum_speed', 'sum_density'):
            arrays[k] = np.concatenate([getattr(p, k) for p in pools], 1)
        elif getattr(pools[0], k) is None:
            arrays[k] = None
        else:
            acc = getattr(pools[0], k).copy()
            for p in pools[1:]:
                acc += getattr(p, k)
            arrays[k] = acc
    opts = dict(pools[0].options)
    opts['frames'] = (0, int(arrays['n'].shape[1]))
    return CrowdStats(arrays, opts)


def compare_crowd_stats(a, b, min_count=50):
    """Distances between two CrowdStats, each pooled over its members first:
      fd_distance = sqrt(sum_b w_b (mean_a,b - mean_b,b)^2 / sum_b w_b), w_b = min(count_a,b, count_b,b), over the bins
                    where both counts are >= min_count (NaN when there is none; fd_bins says how many were used);
      map_distance = sum |m_a - m_b| of the two maps normalised to sum 1 (0 .. 2; None when either side has no map or
                    the boxes / cells differ; NaN when a map is empty);
      mean_speed_diff, mean_density_diff = pooled mean of a - pooled mean of b (means over all focal agent-frames)."""
    if a.options['rho_bins'] != b.options['rho_bins'] or a.options['rho_bin'] != b.options['rho_bin']:
        raise ValueError('compare_crowd_stats: the density bins differ')
    if not same_density(a, b):
        raise ValueError('compare_crowd_stats: the two sides measure density differently ('
                         + ' vs '.join(', '.join(f'{k} {s.options[k]}' for k in DENSITY_KEYS) for s in (a, b)) + ')')
    pa, pb = a.pooled(), b.pooled()
    ca, cb = pa.fd_count[0], pb.fd_count[0]
    use = (ca >= min_count) & (cb >= min_count)
    w = np.minimum(ca, cb)[use].astype(np.float64)
    d = (pa.fd_mean[0] - pb.fd_mean[0])[use]
    fd = float(np.sqrt((w * d * d).sum() / w.sum())) if use.any() else float('nan')
    mp = None
    if pa.map is not None and pb.map is not None and pa.options['box'] == pb.options['box'] \
            and pa.options['cell'] == pb.options['cell']:
        ma, mb = pa.map[0].astype(np.float64), pb.map[0].astype(np.float64)
        sa, sb = ma.sum(), mb.sum()
        mp = float(np.abs(ma / sa - mb / sb).sum()) if sa > 0 and sb > 0 else float('nan')
    mean = lambda p, s, c: float(_nan_div(getattr(p, s).sum(), getattr(p, c).sum()))
    return {'fd_distance': fd, 'fd_bins': int(use.sum()), 'map_distance': mp,
            'mean_speed_diff': mean(pa, 'sum_speed', 'n_speed') - mean(pb, 'sum_speed', 'n_speed'),
            'mean_density_diff': mean(pa, 'sum_density', 'n') - mean(pb, 'sum_density', 'n')}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def parse_box(text):
    """'x0,x1,y0,y1' -> 4 floats; 'auto' -> 'auto'."""
    if text == 'auto':
        return 'auto'
    vals = [float(v) for v in text.split(',')]
    if len(vals) != 4:
        raise ValueError(f'expected x0,x1,y0,y1, got {text!r}')
    return tuple(vals)


def parse_frames(text):
    """'a:b' -> (a, b)"""
    a, b = text.split(':')
    return int(a), int(b)


def auto_box(position, mask, cell):
    """The bounding box of the present agents of (T, N, 2) positions, widened outward to whole cells: x0 = floor(min / h) h,
    x1 = (floor(max / h) + 1) h (the extreme agents are focal), likewise in y."""
    p = np.asarray(position, np.float64).reshape(-1, 2)
    m = (np.asarray(mask).reshape(-1) == 1) & np.isfinite(p).all(1)
    if not m.any():
        raise ValueError('--box auto: no present agent')
    lo, hi = p[m].min(0), p[m].max(0)
    h = float(cell)
    x0, y0 = math.floor(lo[0] / h) * h, math.floor(lo[1] / h) * h
    x1, y1 = (math.floor(hi[0] / h) + 1) * h, (math.floor(hi[1] / h) + 1) * h
    return (x0, x1, y0, y1)


def get_args(argv=None):
    p = argparse.ArgumentParser(description='crowd-dynamics statistics (fundamental diagram, density map, series) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--box', type=str, default=None, help="x0,x1,y0,y1 or 'auto' (bounding box of --ref, else of the first --data)")
    p.add_argument('--radius', type=float, default=0.7)
    p.add_argument('--cell', type=float, default=0.5)
    p.add_argument('--rho_bin', type=float, default=0.25)
    p.add_argument('--rho_bins', type=int, default=24)
    p.add_argument('--density', choices=DENSITIES, default='gaussian', help='the local density (voronoi: --radius is ignored)')
    p.add_argument('--cutoff', type=float, default=None, help='--density voronoi: the cut-off radius of a cell (default 1.0)')
    p.add_argument('--bounds', type=str, default=None,
                   help="--density voronoi: the walkable rectangle x0,x1,y0,y1 that bounds the cells, or 'auto' (the --box in use)")
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=50)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.box = None if args.box is None else parse_box(args.box)
        args.frames = None if args.frames is None else parse_frames(args.frames)
        args.bounds = None if args.bounds is None else parse_box(args.bounds)
        if args.bounds == 'auto' and args.box is None:
            raise ValueError('--bounds auto is the --box in use: give --box')
        check_options(args.radius, None if args.box in (None, 'auto') else args.box, args.cell, args.rho_bin,
                      args.rho_bins, args.frames, density=args.density, cutoff=args.cutoff,
                      bounds=None if args.bounds in (None, 'auto') else args.bounds)
    except ValueError as ex:
        p.error(str(ex))
    return args


def _load(path):
    from .data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(path)
    return raw


def print_diagram(stats, tag, file=sys.stdout):
    pool = stats.pooled()
    edges = stats.bin_edges
    print(f'[crowdstats] {tag}: fundamental diagram (density bin [m^-2]: count, mean speed +- std [m/s])', file=file)
    for k in range(len(edges)):
        c = int(pool.fd_count[0, k])
        if c:
            hi = f'{edges[k + 1]:.2f}' if k + 1 < len(edges) else 'inf'
            print(f'  [{edges[k]:.2f}, {hi}): {c:8d}  {pool.fd_mean[0, k]:.3f} +- {pool.fd_std[0, k]:.3f}', file=file)
    ms = _nan_div(pool.sum_speed.sum(), pool.n_speed.sum())
    md = _nan_div(pool.sum_density.sum(), pool.n.sum())
    print(f'[crowdstats] {tag}: {int(pool.n.sum())} focal agent-frames, mean speed {float(ms):.4f} m/s, '
          f'mean density {float(md):.4f} m^-2', file=file)
    print_dropped(stats, tag, file)


def print_dropped(stats, tag, file=sys.stdout):
    """Says so when Voronoi cells could not be formed (never silently)."""
    if int(stats.dropped.sum()):
        print(f'[crowdstats] {tag}: {int(stats.dropped.sum())} agent-frames left out (Voronoi cell not formed; per member '
              f'{stats.dropped.tolist()})', file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    box = args.box
    if box == 'auto':
        src = ref if ref is not None else raws[0]
        box = auto_box(src.position.numpy(), src.mask_p.numpy(), args.cell)
        print(f'[crowdstats] --box auto: {",".join(f"{v:g}" for v in box)}')
    kw = dict(radius=args.radius, box=box, cell=args.cell, rho_bin=args.rho_bin, rho_bins=args.rho_bins,
              frames=args.frames)
    if args.density != 'gaussian':
        kw.update(density=args.density, cutoff=args.cutoff, bounds=box if args.bounds == 'auto' else args.bounds)
    data = merge([crowd_stats_of_raw(r, **kw) for r in raws])
    print_diagram(data, 'data')
    out = {'data': data.to_json()}
    if ref is not None:
        rs = crowd_stats_of_raw(ref, **kw)
        print_diagram(rs, 'ref')
        cmp = compare_crowd_stats(data, rs, args.min_count)
        print('[crowdstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                                      for k, v in cmp.items()))
        out['ref'] = rs.to_json()
        out['compare'] = {k: (_json_float(v) if isinstance(v, float) else v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[crowdstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
