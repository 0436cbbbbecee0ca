"""Group statistics of crowds: who walks with whom, group size, spacing and formation.  Most pedestrians in a
street walk with someone (Moussaid et al. 2010); groups walk side by side and more slowly than singles.  The siblings
(crowdstats, pairstats, flowstats, trackstats, obstaclestats, linestats) cannot see it: pair statistics forget identities
after one frame and track statistics follow one agent at a time.  This family keeps the identities of a pair through time:
a pair sweep on the device (piml_group_pairs), the link rule and a union-find on the host (or, with components='device',
in piml_group_components: DESIGN 4.28), and the member statistics of the linked pairs on the device again
(piml_group_members); ops_metrics.group_stats_frames runs the three for all members.

    python -m piml_amd.groupstats --data sim_0.npy [sim_1.npy ...] [--ref recorded.npy] [--frames a:b] [--radius 2.0]
                                  [--dv-max 0.5] [--min-time 2.0] [--share 0.8] [--out groups.json]

Definitions.  P (S, T, N, 2) and M (S, T, N) float32, plus dt; velocities are not an input: as in trackstats and linestats,
slot n of a member is one agent for the whole run.  Agent i takes part at (member s, frame t) when its mask is 1, both
coordinates are finite and below 65536 in magnitude and i < n_active[s]; t is an index into the window frames = (a, b) of T'
frames.  A step (i, t) exists when i takes part at t and at t + 1, and t + 1 < T'; its displacement is
u_i(t) = p_i(t+1) - p_i(t), in metres per frame, float32.  All arithmetic is float32 with separately rounded products, true
square roots and divisions and no contraction; Q = 2^20.  The host makes each threshold once in float64 and rounds it once
to float32: r2 = f32(radius^2), dv2 = f32((dv_max dt)^2), vm2 = f32((v_min dt)^2) (ops_metrics.group_thresholds).
  A pair-frame (i, j, t), i < j, exists when both steps exist at t; it adds 1 to co[i, j].  With e = p_j(t) - p_i(t) and
      g = u_j(t) - u_i(t) it is together when ex ex + ey ey < r2, gx gx + gy gy < dv2, |u_i|^2 >= vm2 and |u_j|^2 >= vm2
      (each sum the x term plus the y term); a together pair-frame adds 1 to near[i, j].
  min_frames = max(1, ceil(min_time / dt)).  A pair is a candidate when near >= min_frames, and a candidate is a link when
      near 1024 >= share_q co, share_q = round(share 1024), in integers.
  A track is eligible when it has at least min_frames steps (every end of a candidate is).  Groups are the connected
      components of the links over the eligible tracks of a member.  Chaining is intended -- i-j and j-k linked makes one
      group of three, also when i and k are never together --, and it over-merges in dense crowds, where a walker between two
      groups joins them.
Device, pass 1: edges, rows (member, i, j, co, near) of every candidate, sorted; n_edges (S); trk_steps (S, N) the steps of
  each track; trk_path (S, N) the sum of llrintf(sqrtf(|u|^2) Q) over them; pairs, together (S) the pair-frames swept and
  the together ones.  Its cost grows as S N^2 times the frames present.
The host half, integers only (host_rows): links, candidates (S); group_id (S, N) int32 the smallest slot of the track's
  component, -1 for an ineligible track; size_tracks (S, g_max + 1): at index k >= 1 the eligible tracks in groups of size
  min(k, g_max), g_max = 8, index 0 stays 0; size_path, size_steps: the sums of trk_path and trk_steps of those tracks (the
  speed by group size is path / steps / Q / dt); slices (S) the frames of the window.
Device, pass 2, over every together pair-frame of a link, with d2 = ex ex + ey ey, d = sqrtf(d2), w = u_i + u_j,
  w2 = wx wx + wy wy: dist (S, r_bins + 1) by min(floor(d / r_bin), r_bins); dist_sum (S) the sum of llrintf(d Q); abreast
  (S, a_bins) by min(floor(c a_bins), a_bins - 1), c = fabsf(ex wx + ey wy) / (sqrtf(d2) sqrtf(w2)): bin 0 is side by side,
  the last bin in file; abreast_skipped (S) the pair-frames with d2 == 0 or w2 == 0 instead; link_frames (S) the together
  pair-frames of the links (= dist.sum(-1) = the sum of near over the links)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from .crowdstats import (_bounds, _f32, _json_float, _json_floats, _l1, _load, _nan_div, _total, _window,
                         member_indices, parse_frames)

JSON_VERSION = 1
Q = 1 << 20
G_MAX = 8
SHARE_UNIT = 1024
DEVICE = ('pairs', 'together', 'dist', 'dist_sum', 'abreast', 'abreast_skipped', 'link_frames')
HOST = ('candidates', 'links', 'size_tracks', 'size_path', 'size_steps')
ADDITIVE = DEVICE + HOST + ('slices',)
TRACK_ROWS = ('trk_steps', 'trk_path', 'group_id', 'n_edges')
ARRAYS = ADDITIVE + TRACK_ROWS + ('edges',)
OPTION_KEYS = ('dt', 'radius', 'dv_max', 'v_min', 'min_time', 'share', 'r_bin', 'r_bins', 'a_bins', 'g_max')
DEFAULTS = dict(dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8, r_bin=0.1, r_bins=20, a_bins=10)


def check_options(dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8, r_bin=0.1, r_bins=20, a_bins=10,
                  frames=None, max_edges=None, T=None, N=None):
    """ValueError on a bad option; returns frames (a, b) or None."""
    from .ops_metrics import GROUP_MAX_BINS, GROUP_MAX_FRAMES, GROUP_MAX_N, group_thresholds
    for name, x in (('dt', dt), ('radius', radius), ('dv_max', dv_max), ('min_time', min_time), ('r_bin', r_bin)):
        if isinstance(x, bool) or not (math.isfinite(float(x)) and float(x) > 0 and math.isfinite(_f32(x)) and _f32(x) > 0):
            raise ValueError(f'{name} must be a positive number, got {x}')
    if isinstance(v_min, bool) or not (math.isfinite(float(v_min)) and float(v_min) >= 0):
        raise ValueError(f'v_min must be a number >= 0, got {v_min}')
    if isinstance(share, bool) or not 0 < float(share) <= 1:
        raise ValueError(f'share must be in (0, 1], got {share}')
    if float(radius) > 1024:
        raise ValueError(f'radius must be at most 1024 m, got {radius}')
    for name, x in (('r_bins', r_bins), ('a_bins', a_bins)):
        if isinstance(x, bool) or int(x) != x or not 1 <= int(x) <= GROUP_MAX_BINS:
            raise ValueError(f'{name} must be an integer in 1..{GROUP_MAX_BINS}, got {x}')
    r2, dv2, vm2, min_frames, _ = group_thresholds(dt, radius, dv_max, v_min, min_time, share)
    if not (r2 > 0 and dv2 > 0 and all(math.isfinite(x) for x in (r2, dv2, vm2))) or min_frames > GROUP_MAX_FRAMES:
        raise ValueError(f'group_stats: the thresholds (radius^2, (dv_max dt)^2, (v_min dt)^2) = ({r2}, {dv2}, {vm2}) must be '
                         f'finite and the first two positive in float32, min_time / dt at most {GROUP_MAX_FRAMES}')
    if max_edges is not None and (isinstance(max_edges, bool) or int(max_edges) != max_edges or not 1 <= int(max_edges) < 2 ** 31):
        raise ValueError(f'max_edges must be None or a positive integer, got {max_edges}')
    frames = _window(frames, T)
    span = (frames[1] - frames[0]) if frames is not None else (T or 0)
    if span > GROUP_MAX_FRAMES:
        raise ValueError(f'group_stats: {span} frames in the window (at most {GROUP_MAX_FRAMES})')
    if N is not None:
        if N > GROUP_MAX_N:
            raise ValueError(f'group_stats: {N} slots per frame (at most {GROUP_MAX_N})')
        if not math.sqrt(r2) * Q * 0.5 * N * N * span < 2.0 ** 63:
            raise ValueError(f'group_stats: {N} slots x {span} frames could overflow the 64-bit distance sum (radius {radius})')
    return frames


def host_rows(rows, min_frames, share_q, g_max=G_MAX):
    """The host half: candidates, links (S) int64, group_id (S, N) int32 and size_tracks, size_path, size_steps
    (S, g_max + 1) int64 from the integer rows edges (E, 5) (member, i, j, co, near), trk_steps and trk_path (S, N) (module
    docstring): the link rule, a union-find per member, the sizes."""
    edges = np.asarray(rows['edges'], np.int64).reshape(-1, 5)
    steps, path = np.asarray(rows['trk_steps'], np.int64), np.asarray(rows['trk_path'], np.int64)
    S, N = steps.shape
    G = int(g_max)
    out = dict(candidates=np.bincount(edges[:, 0], minlength=S).astype(np.int64)[:S], links=np.zeros(S, np.int64),
               group_id=np.full((S, N), -1, np.int32), size_tracks=np.zeros((S, G + 1), np.int64),
               size_path=np.zeros((S, G + 1), np.int64), size_steps=np.zeros((S, G + 1), np.int64))
    link = edges[:, 4] * SHARE_UNIT >= int(share_q) * edges[:, 3]
    for s in range(S):
        parent = np.arange(N)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        mine = edges[link & (edges[:, 0] == s)]
        out['links'][s] = mine.shape[0]
        for i, j in mine[:, 1:3]:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)                  # the root is the smallest slot of the component
        eligible = steps[s] >= int(min_frames)
        root = np.array([find(n) for n in range(N)], np.int64)
        out['group_id'][s] = np.where(eligible, root, -1)
        size = np.bincount(root[eligible], minlength=N) if N else np.zeros(0, np.int64)
        k = np.minimum(size[root], G)
        for name, val in (('size_tracks', np.ones(N, np.int64)), ('size_path', path[s]), ('size_steps', steps[s])):
            np.add.at(out[name][s], k[eligible], val[eligible])
    return out


class GroupStats:
    """The group statistics of S members (numpy int64; module docstring): pairs, together, candidates, links, dist_sum,
    abreast_skipped, link_frames, slices (S); dist (S, r_bins + 1); abreast (S, a_bins); size_tracks, size_path, size_steps
    (S, g_max + 1); and, as they come from the device and the host half, trk_steps, trk_path (S, N), group_id (S, N), n_edges
    (S) and edges (E, 5), rows (member, i, j, co, near) sorted (None once statistics are pooled or merged: tracks of
    different members do not add).  options: dt, radius, dv_max, v_min, min_time, share, r_bin, r_bins, a_bins, g_max,
    min_frames, share_q and frames (None once statistics of different windows are merged).  The derived quantities are those
    of the statistics pooled over the members."""

    def __init__(self, arrays, options):
        for k in ARRAYS:
            v = arrays.get(k)
            setattr(self, k, None if v is None else np.asarray(v, np.int64))
        if self.edges is not None:
            self.edges = self.edges.reshape(-1, 5)
        self.options = dict(options)

    @property
    def members(self):
        return self.pairs.shape[0]

    @property
    def dt(self):
        return _f32(self.options['dt'])

    def select(self, members):
        """The same statistics restricted to the members of a list of indices (0 .. members - 1, in the list's order, repeats
        allowed), with the same options: `.select(group).pooled()` pools one group.  IndexError on an index out of range."""
        idx = member_indices(members, self.members)
        arrays = {k: None if getattr(self, k) is None else getattr(self, k)[idx] for k in ADDITIVE + TRACK_ROWS}
        if self.edges is not None:
            parts = []
            for new, m in enumerate(idx):
                rows = self.edges[self.edges[:, 0] == m].copy()
                rows[:, 0] = new
                parts.append(rows)
            arrays['edges'] = np.concatenate(parts) if parts else np.zeros((0, 5), np.int64)
        return GroupStats(arrays, self.options)

    def member(self, m):
        """Member m as a one-member GroupStats."""
        return self.select([m])

    def pooled(self):
        """The sum over members, added in member order: a one-member GroupStats without track rows."""
        return GroupStats({k: _total(getattr(self, k)) for k in ADDITIVE}, self.options)

    @staticmethod
    def merge(stats):
        """Several GroupStats with the same options (frames aside) as one member: each pooled, added in list order."""
        return merge(stats)

    def groups(self, member=0):
        """The groups of two or more of one member: lists of slots, each ascending, ordered by their smallest slot."""
        if self.group_id is None:
            raise ValueError('groups: the statistics were pooled or merged')
        gid = self.group_id[member]
        out = [np.nonzero(gid == r)[0].tolist() for r in np.unique(gid[gid >= 0])]
        return [g for g in out if len(g) >= 2]

    # -- derived, float64, of the pooled statistics
    def eligible_tracks(self):
        return int(self.pooled().size_tracks[0].sum())

    def group_fraction(self):
        """the share of eligible tracks that walk in a group of two or more (NaN without an eligible track)"""
        c = self.pooled().size_tracks[0]
        return float(_nan_div(c[2:].sum(), c.sum()))

    def size_distribution(self):
        """(g_max + 1,) the share of eligible tracks by the size of their group (index 0 is 0, index g_max: that size or more)"""
        c = self.pooled().size_tracks[0]
        return _nan_div(c, np.full(c.shape, c.sum()))

    def speed_by_size(self):
        """(g_max + 1,) the mean speed of the tracks by the size of their group, path / steps / Q / dt, m/s (NaN without a step)"""
        p = self.pooled()
        return _nan_div(p.size_path[0] / float(Q) / self.dt, p.size_steps[0])

    def speed_ratio(self):
        """the mean speed of the tracks in groups of two or more over that of the single tracks (NaN without either)"""
        p = self.pooled()
        grouped = _nan_div(p.size_path[0, 2:].sum(), p.size_steps[0, 2:].sum())
        single = _nan_div(p.size_path[0, 1], p.size_steps[0, 1])
        return float(_nan_div(grouped, single))

    def member_distance_density(self):
        """(r_bins,) together pair-frames of the links per pair-frame and per metre of distance (the rest: beyond the range)"""
        c = self.pooled().dist[0]
        return _nan_div(c[:-1], np.full(c[:-1].shape, c.sum() * _f32(self.options['r_bin'])))

    def mean_member_distance(self):
        """dist_sum / (Q link_frames), metres"""
        p = self.pooled()
        return float(_nan_div(p.dist_sum[0] / float(Q), p.link_frames[0]))

    def abreast_density(self):
        """(a_bins,) together pair-frames of the links per pair-frame and per unit of c = |cos| of the angle between the line of
        the pair and its walking direction: bin 0 side by side, the last bin in file"""
        c = self.pooled().abreast[0]
        return _nan_div(c * float(c.shape[0]), np.full(c.shape, c.sum()))

    def summary(self):
        p = self.pooled()
        return {'eligible_tracks': self.eligible_tracks(), 'links': int(p.links[0]), 'candidates': int(p.candidates[0]),
                'pairs': int(p.pairs[0]), 'together': int(p.together[0]), 'link_frames': int(p.link_frames[0]),
                'group_fraction': _json_float(self.group_fraction()), 'size_tracks': p.size_tracks[0].tolist(),
                'size_distribution': _json_floats(self.size_distribution()), 'speed_by_size': _json_floats(self.speed_by_size()),
                'speed_ratio': _json_float(self.speed_ratio()), 'mean_member_distance': _json_float(self.mean_member_distance()),
                'abreast_density': _json_floats(self.abreast_density()), 'slices': int(p.slices[0])}

    def to_json(self, path=None):
        """A JSON-ready dict of the options, the raw arrays and the pooled derived summary; written to path if given."""
        o = self.options
        d = {'version': JSON_VERSION, 'options': {**o, 'frames': None if o.get('frames') is None else list(o['frames'])},
             'arrays': {k: None if getattr(self, k) is None else getattr(self, k).tolist() for k in ARRAYS},
             'pooled': self.summary()}
        if path is not None:
            with open(path, 'w') as fh:
                json.dump(d, fh)
        return d

    @classmethod
    def from_json(cls, src):
        """A GroupStats from what to_json wrote (a path or the dict)."""
        if not isinstance(src, dict):
            with open(src) as fh:
                src = json.load(fh)
        if src.get('version') != JSON_VERSION:
            raise ValueError(f'group stats JSON version {src.get("version")!r} (expected {JSON_VERSION})')
        o = dict(src['options'])
        o['frames'] = None if o.get('frames') is None else tuple(o['frames'])
        return cls(src['arrays'], o)


def merge(stats):
    """Several GroupStats with the same options (frames aside) as one member: each pooled, added in list order; no track rows."""
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
    return GroupStats(arrays, opts)


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


def make_options(dt, radius, dv_max, v_min, min_time, share, r_bin, r_bins, a_bins, frames):
    """the options dict of a GroupStats (min_frames and share_q included)"""
    from .ops_metrics import group_thresholds
    _, _, _, min_frames, share_q = group_thresholds(dt, radius, dv_max, v_min, min_time, share)
    return dict(dt=float(dt), radius=float(radius), dv_max=float(dv_max), v_min=float(v_min), min_time=float(min_time),
                share=float(share), r_bin=float(r_bin), r_bins=int(r_bins), a_bins=int(a_bins), g_max=G_MAX,
                min_frames=min_frames, share_q=share_q, frames=frames)


def group_stats(P, M, dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8, r_bin=0.1, r_bins=20, a_bins=10,
                frames=None, n_active=None, max_edges=None, components='host'):
    """The group statistics of positions P (S, T, N, 2) and presence M (S, T, N) -- (T, N, .) is one member -- for all
    members at once: GroupStats.  dt the seconds per frame; two agents are together in a frame when they are closer than
    `radius` m, their velocities differ by less than `dv_max` m/s and both move at `v_min` m/s or more; a pair is linked when
    it is together for at least `min_time` s and for at least `share` of the frames both are present.  frames (a, b) the
    window; n_active (S) ints: member s's slots at or past n_active[s] never held an agent and are not swept; max_edges the
    cap on the candidate pairs per member (None: min(N (N - 1) / 2, 2^20); ValueError naming the count needed when it is too
    small).  components: 'host' (the default) runs the link rule, the components and the sizes in host_rows; 'device' runs
    them in piml_group_components between the two passes -- the same GroupStats array for array, without the
    interpreter loop per member.  Every option is checked on the host before anything is launched."""
    if components not in ('host', 'device'):
        raise ValueError(f"components: 'host' or 'device' expected, got {components!r}")
    from . import ops_metrics
    shape = tuple(getattr(P, 'shape', ()))
    T, N = (shape[-3], shape[-2]) if len(shape) in (3, 4) else (None, None)
    frames = check_options(dt, radius, dv_max, v_min, min_time, share, r_bin, r_bins, a_bins, frames, max_edges, T, N)
    P, M = _promote(P, M)
    S, T, N = P.shape[:3]
    frames = frames or (0, T)
    n_active = _bounds(n_active, S, N, P.device)
    out = ops_metrics.group_stats_frames(P, M, dt, radius, dv_max, v_min, min_time, share, r_bin, int(r_bins), int(a_bins),
                                         frames, n_active, max_edges, components, G_MAX)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    opts = make_options(dt, radius, dv_max, v_min, min_time, share, r_bin, r_bins, a_bins, frames)
    if components == 'device':
        if host.pop('status').any():
            raise RuntimeError('group_stats: piml_group_components did not settle (status != 0)')
    else:
        host.update(host_rows(host, opts['min_frames'], opts['share_q']))
    host['slices'] = np.full(S, frames[1] - frames[0], np.int64)
    return GroupStats(host, opts)


def group_stats_of_raw(raw_data, **kw):
    """group_stats of a loaded clip (piml_amd.data.data.RawData: position, mask_p), one member; dt is the clip's time_unit
    unless given."""
    kw.setdefault('dt', float(raw_data.time_unit))
    return group_stats(raw_data.position, raw_data.mask_p, **kw)


def _hist_l1(ha, hb, min_count):
    """_l1 of the shares of two histograms; NaN with fewer than min_count items on either side"""
    na, nb = int(ha.sum()), int(hb.sum())
    if min(na, nb) < max(int(min_count), 1):
        return float('nan')
    return _l1(ha / na, hb / nb)


def compare_group_stats(a, b, min_count=20):
    """Distances between two GroupStats, each pooled over its members:
      group_fraction_diff = |group_fraction a - b|, and size_l1 = sum |share_a - share_b| over the group sizes (0 .. 2), with
          at least min_count eligible tracks on both sides;
      member_distance_l1, abreast_l1 = sum |share_a - share_b| over the bins of dist (the open last bin included) and of
          abreast, with at least min_count such pair-frames on both sides;
      speed_ratio_diff = |speed_ratio a - b|, with at least min_count single and min_count grouped tracks on both sides.
    A term without enough data is NaN.  ValueError when the two were taken with different options (dt, radius, dv_max, v_min,
    min_time, share, the bins)."""
    for k in OPTION_KEYS:
        if a.options[k] != b.options[k]:
            raise ValueError(f'compare_group_stats: the options differ ({k}: {a.options[k]} vs {b.options[k]})')
    pa, pb = a.pooled(), b.pooled()
    ta, tb = pa.size_tracks[0], pb.size_tracks[0]
    floor = max(int(min_count), 1)
    enough = min(ta.sum(), tb.sum()) >= floor
    both = min(ta[1], tb[1], ta[2:].sum(), tb[2:].sum()) >= floor
    return {'group_fraction_diff': abs(a.group_fraction() - b.group_fraction()) if enough else float('nan'),
            'size_l1': _hist_l1(ta, tb, min_count), 'member_distance_l1': _hist_l1(pa.dist[0], pb.dist[0], min_count),
            'abreast_l1': _hist_l1(pa.abreast[0], pb.abreast[0], min_count),
            'speed_ratio_diff': abs(a.speed_ratio() - b.speed_ratio()) if both else float('nan')}


# ---------------------------------------------------------------------------------------------------------------------
# command line

def get_args(argv=None):
    p = argparse.ArgumentParser(description='group statistics (who walks with whom, group size, spacing, formation) of clips')
    p.add_argument('--data', nargs='+', required=True, help='v2.2 clips (simulated or recorded), pooled together')
    p.add_argument('--ref', type=str, default=None, help='a clip to compare against')
    p.add_argument('--dt', type=float, default=None, help="seconds per frame (default: each clip's time_unit)")
    p.add_argument('--radius', type=float, default=DEFAULTS['radius'], help='together: closer than this, m')
    p.add_argument('--dv-max', dest='dv_max', type=float, default=DEFAULTS['dv_max'],
                   help='together: velocities differ by less than this, m/s')
    p.add_argument('--v-min', dest='v_min', type=float, default=DEFAULTS['v_min'], help='together: both move at this speed or more, m/s')
    p.add_argument('--min-time', dest='min_time', type=float, default=DEFAULTS['min_time'], help='linked: together at least this long, s')
    p.add_argument('--share', type=float, default=DEFAULTS['share'],
                   help='linked: together in at least this share of the frames both are present')
    p.add_argument('--r_bin', type=float, default=DEFAULTS['r_bin'])
    p.add_argument('--r_bins', type=int, default=DEFAULTS['r_bins'])
    p.add_argument('--a_bins', type=int, default=DEFAULTS['a_bins'])
    p.add_argument('--frames', type=str, default=None, help="'a:b' (frames a .. b-1 of every clip)")
    p.add_argument('--min_count', type=int, default=20)
    p.add_argument('--out', type=str, default=None, help='JSON of the pooled statistics (and the comparison)')
    args = p.parse_args(argv)
    try:
        args.frames = None if args.frames is None else parse_frames(args.frames)
        check_options(0.08 if args.dt is None else args.dt, args.radius, args.dv_max, args.v_min, args.min_time, args.share,
                      args.r_bin, args.r_bins, args.a_bins, args.frames)
    except ValueError as ex:
        p.error(str(ex))
    return args


def print_group_stats(stats, tag, file=sys.stdout):
    p = stats.pooled()
    print(f'[groupstats] {tag}: {stats.eligible_tracks()} eligible tracks, {int(p.links[0])} links of {int(p.candidates[0])} '
          f'candidates, {int(p.together[0])} of {int(p.pairs[0])} pair-frames together, over {int(p.slices[0])} frames', file=file)
    print(f'  group fraction {stats.group_fraction():.4f}, tracks by group size {p.size_tracks[0, 1:].tolist()}', file=file)
    print('  speed by group size [m/s] ' + ', '.join(f'{v:.3f}' for v in stats.speed_by_size()[1:]) +
          f'; grouped / single {stats.speed_ratio():.4f}', file=file)
    print(f'  mean member distance {stats.mean_member_distance():.3f} m over {int(p.link_frames[0])} pair-frames; abreast density '
          + ', '.join(f'{v:.2f}' for v in stats.abreast_density()), file=file)


def main(argv=None):
    args = get_args(argv)
    raws = [_load(p) for p in args.data]
    ref = _load(args.ref) if args.ref else None
    kw = dict(radius=args.radius, dv_max=args.dv_max, v_min=args.v_min, min_time=args.min_time, share=args.share,
              r_bin=args.r_bin, r_bins=args.r_bins, a_bins=args.a_bins, frames=args.frames)
    if args.dt is not None:
        kw['dt'] = args.dt
    data = merge([group_stats_of_raw(r, **kw) for r in raws])
    print_group_stats(data, 'data')
    out = {'data': data.to_json()}
    if ref is not None:
        rs = group_stats_of_raw(ref, **kw)
        print_group_stats(rs, 'ref')
        cmp = compare_group_stats(data, rs, args.min_count)
        print('[groupstats] data vs ref: ' + ', '.join(f'{k} {v:.4g}' for k, v in cmp.items()))
        out['ref'] = rs.to_json()
        out['compare'] = {k: _json_float(v) for k, v in cmp.items()}
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh)
        print(f'[groupstats] wrote {os.path.abspath(args.out)}')
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
