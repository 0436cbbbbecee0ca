"""Evaluation-metric operators over the C ABI (include/piml_hip.h: piml_sinkhorn_frames, piml_mmd_frames).

Entropic OT and multi-kernel MMD of point clouds, every frame in one launch.  Like every operator of piml_amd they
require float32 GPU tensors and raise PimlHipError on CPU ones; functions/metrics.py builds the reference's interface on
them."""
import math

import numpy as np
import torch

from . import _lib
from .ops import _gpu_f32, _ptr, _stream


def _frames(name, t):
    """(*c, n, 2) -> contiguous (F, n, 2) and the leading shape (n <= 4096 is the library's check)."""
    t = _gpu_f32(name, t.detach())
    if t.dim() < 2 or t.shape[-1] != 2:
        raise ValueError(f'{name}: expected (*c, n, 2), got {tuple(t.shape)}')
    lead = t.shape[:-2]
    return t.reshape(lead.numel(), t.shape[-2], 2), lead


def _mask(name, mask, x):
    """None, or (*c, n) presence (non-zero = present) -> uint8 (F, n) on x's device."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.device != x.device:
        raise _lib.PimlHipError(f'{name}: expected a tensor on {x.device}, got {getattr(mask, "device", type(mask))}')
    if mask.numel() != x.shape[0] * x.shape[1]:
        raise ValueError(f'{name}: {tuple(mask.shape)} does not match {x.shape[0]} frames of {x.shape[1]} points')
    return (mask != 0).to(torch.uint8).reshape(x.shape[0], x.shape[1])


def _pair(x, y, mask_x, mask_y):
    x, lead = _frames('x', x)
    y, lead_y = _frames('y', y)
    if lead != lead_y:
        raise ValueError(f'x and y frames differ: {tuple(lead)} vs {tuple(lead_y)}')
    if x.device != y.device:
        raise ValueError('x and y on different devices')
    return x, y, _mask('mask_x', mask_x, x), _mask('mask_y', mask_y, y), lead


def sinkhorn_frames(x, y, mask_x=None, mask_y=None, eps=0.1, max_iter=100, thresh=0.1, want_potentials=False):
    """Entropic OT cost of every frame (SinkhornDistance, src/functions/metrics.py:107-187, per frame): x (*c, n, 2),
    y (*c, m, 2), optional presence masks (*c, n) / (*c, m).  Returns (cost (*c) float32, iters (*c) int32) and, with
    want_potentials, the potentials u (*c, n) and v (*c, m) (0 at absent points)."""
    x, y, mx, my, lead = _pair(x, y, mask_x, mask_y)
    F, n, m = x.shape[0], x.shape[1], y.shape[1]
    cost = torch.empty(F, device=x.device, dtype=torch.float32)
    iters = torch.empty(F, device=x.device, dtype=torch.int32)
    u = torch.empty(F, n, device=x.device, dtype=torch.float32) if want_potentials else None
    v = torch.empty(F, m, device=x.device, dtype=torch.float32) if want_potentials else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().piml_sinkhorn_frames(_ptr(x), _ptr(y), _ptr(mx), _ptr(my), F, n, m, float(eps), int(max_iter),
                                                   float(thresh), _ptr(cost), _ptr(iters), _ptr(u), _ptr(v), _stream()),
                   'piml_sinkhorn_frames')
    out = (cost.reshape(lead), iters.reshape(lead))
    if want_potentials:
        out += (u.reshape(*lead, n), v.reshape(*lead, m))
    return out


def mmd_frames(x, y, mask_x=None, mask_y=None, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """Multi-kernel Gaussian MMD of every frame (MaximumMeanDiscrepancy, src/functions/metrics.py:207-273, per frame),
    evaluated in float64: x (*c, n, 2), y (*c, m, 2), optional presence masks.  fix_sigma follows Python truthiness
    (None or 0: the bandwidth of the data).  Returns (*c) float32."""
    x, y, mx, my, lead = _pair(x, y, mask_x, mask_y)
    F, n, m = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty(F, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().piml_mmd_frames(_ptr(x), _ptr(y), _ptr(mx), _ptr(my), F, n, m, float(kernel_mul),
                                              int(kernel_num), float(fix_sigma) if fix_sigma else 0.0, _ptr(out), _stream()),
                   'piml_mmd_frames')
    return out.reshape(lead)


def _stats_setup(named, frames, n_active):
    """What every statistics wrapper checks first.  named: its float32 inputs by name -- P (S, T, N, 2), V like P when the
    call has one, M (S, T, N), then any further ones, whose shapes are the caller's to check -- in the order the messages
    list them.  Returns the contiguous tensors in that order, (S, T, N, a, b) with the window (a, b) of `frames`, the device
    and n_active, contiguous; ValueError unless every tensor, n_active included, is on P's device."""
    t = {k: _gpu_f32(k, x) for k, x in named.items()}
    P, V, M = t['P'], t.get('V'), t['M']
    if P.dim() != 4 or P.shape[-1] != 2 or (V is not None and V.shape != P.shape) or M.shape != P.shape[:3]:
        if V is None:
            raise ValueError(f'expected P (S, T, N, 2) and M (S, T, N), got {tuple(P.shape)}, {tuple(M.shape)}')
        raise ValueError(f'expected P, V (S, T, N, 2) and M (S, T, N), got {tuple(P.shape)}, {tuple(V.shape)}, '
                         f'{tuple(M.shape)}')
    dev = P.device
    if any(x.device != dev for x in t.values()):
        names = list(t)
        raise ValueError(f'{", ".join(names[:-1])} and {names[-1]} on different devices')
    S, T, N = P.shape[:3]
    a, b = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    if n_active is not None:
        if not isinstance(n_active, torch.Tensor) or n_active.device != dev or n_active.dtype != torch.int32 \
                or tuple(n_active.shape) != (S,):
            raise ValueError(f'n_active: expected an int32 ({S},) tensor on {dev}')
        n_active = n_active.contiguous()
    return tuple(t.values()), (S, T, N, a, b), dev, n_active


def _stats_new(idle, dev, ws_bytes=None):
    """The allocator of a call's outputs and its workspace (None without ws_bytes).  A call with nothing to do leaves its
    outputs alone, so it is handed zeros."""
    ws = None if ws_bytes is None else torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    return (torch.zeros if idle else torch.empty), ws


CROWD_MAX_BINS = 256          # piml_crowd_stats' limit on rho_bins


def _crowd_setup(P, V, M, box, grid, rho_bins, frames, return_density, n_active):
    """What the two crowd-statistics calls share: checked inputs, the frame range, the box as numbers and the outputs."""
    (P, V, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, V=V, M=M), frames, n_active)
    Tp, B = b - a, int(rho_bins)
    gx, gy = (1, 1) if box is None else (int(grid[0]), int(grid[1]))
    rect = (0.0, 0.0, 0.0, 0.0) if box is None else tuple(float(v) for v in box)
    i64, f64 = dict(device=dev, dtype=torch.int64), dict(device=dev, dtype=torch.float64)
    shape_s, shape_b = (S, max(Tp, 0)), (S, max(B, 0))
    out = dict(n=torch.empty(shape_s, **i64), n_speed=torch.empty(shape_s, **i64), sum_speed=torch.empty(shape_s, **f64),
               sum_density=torch.empty(shape_s, **f64), fd_count=torch.empty(shape_b, **i64),
               fd_sum=torch.empty(shape_b, **f64), fd_sum2=torch.empty(shape_b, **f64),
               map=torch.empty(S, gy, gx, **i64) if box is not None else None,
               density=torch.empty(S, max(Tp, 0), N, device=dev, dtype=torch.float32) if return_density else None)
    return P, V, M, n_active, (S, T, N, a, b), (Tp, B), rect, (gx, gy), out


def _crowd_out_ptrs(out):
    return tuple(_ptr(out[k]) for k in ('n', 'n_speed', 'sum_speed', 'sum_density', 'fd_count', 'fd_sum', 'fd_sum2', 'map',
                                        'density'))


def crowd_stats_frames(P, V, M, radius=0.7, box=None, grid=None, cell=0.5, rho_bin=0.25, rho_bins=24, frames=None,
                       return_density=False, n_active=None):
    """The device half of piml_amd.crowdstats.crowd_stats (piml_crowd_stats): P, V (S, T, N, 2) and M
    (S, T, N) float32 GPU tensors, box (x0, x1, y0, y1) with its grid (gx, gy) or None, frames (a, b) or None,
    n_active (S) int32 GPU tensor or None.  Returns a dict of GPU tensors -- n, n_speed (S, T') int64, sum_speed,
    sum_density (S, T') float64, fd_count (S, B) int64, fd_sum, fd_sum2 (S, B) float64, map (S, gy, gx) int64 or None,
    density (S, T', N) float32 or None -- with no host synchronisation (capturable in a graph)."""
    P, V, M, n_active, dims, (Tp, B), rect, (gx, gy), out = _crowd_setup(P, V, M, box, grid, rho_bins, frames,
                                                                         return_density, n_active)
    L = _lib.lib()
    _, ws = _stats_new(False, P.device, L.piml_crowd_stats_workspace_bytes(dims[0], max(Tp, 0), max(B, 0)))
    with torch.cuda.device(P.device):
        _lib.check(L.piml_crowd_stats(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), *dims, float(radius),
                                      int(box is not None), *rect, float(cell), gx, gy, float(rho_bin), B,
                                      *_crowd_out_ptrs(out), _ptr(ws), ws.numel(), _stream()),
                   'piml_crowd_stats')
    return out


def crowd_stats_voronoi_frames(P, V, M, cutoff=1.0, dirs=None, bounds=None, box=None, grid=None, cell=0.5, rho_bin=0.25,
                               rho_bins=24, frames=None, return_density=False, n_active=None):
    """crowd_stats_frames on the Voronoi density (piml_crowd_stats_voronoi): cutoff the cells' cut-off radius,
    dirs (sides, 2) float32 unit vectors on the host (crowdstats.voronoi_dirs), bounds (x0, x1, y0, y1) the walkable
    rectangle or None.  The same dict, and dropped (S) int64: the focal agents whose cell could not be formed."""
    import ctypes
    import numpy as np
    P, V, M, n_active, dims, (Tp, B), rect, (gx, gy), out = _crowd_setup(P, V, M, box, grid, rho_bins, frames,
                                                                         return_density, n_active)
    S, N = dims[0], dims[2]
    dirs = np.ascontiguousarray(dirs, np.float32)
    if dirs.ndim != 2 or dirs.shape[1] != 2:
        raise ValueError(f'dirs: expected (sides, 2), got {dirs.shape}')
    out['dropped'] = torch.empty(S, device=P.device, dtype=torch.int64)
    brect = (0.0, 0.0, 0.0, 0.0) if bounds is None else tuple(float(v) for v in bounds)
    L = _lib.lib()
    _, ws = _stats_new(False, P.device, L.piml_crowd_stats_voronoi_workspace_bytes(S, max(Tp, 0), N, max(B, 0)))
    with torch.cuda.device(P.device):
        _lib.check(L.piml_crowd_stats_voronoi(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), *dims, float(cutoff),
                                              dirs.ctypes.data_as(ctypes.c_void_p), int(dirs.shape[0]),
                                              int(bounds is not None), *brect, int(box is not None), *rect, float(cell),
                                              gx, gy, float(rho_bin), B, *_crowd_out_ptrs(out), _ptr(out['dropped']),
                                              _ptr(ws), ws.numel(), _stream()),
                   'piml_crowd_stats_voronoi')
    return out


PAIR_MAX_BINS = 256           # piml_pair_stats' limits on tau_bins / r_bins, the number of lags and the slots per frame
PAIR_MAX_LAGS = 8
PAIR_MAX_N = 65536


def pair_stats_frames(P, V, M, radius=0.5, lags=(64, 128, 192), tau_bin=0.1, tau_bins=100, r_bin=0.05, r_bins=100,
                      r_max=None, box=None, frames=None, n_active=None):
    """The device half of piml_amd.pairstats.pair_stats (piml_pair_stats): P, V (S, T, N, 2) and M (S, T, N)
    float32 GPU tensors, lags a sequence of K positive ascending ints, r_max a distance or None, box (x0, x1, y0, y1) or
    None, frames (a, b) or None, n_active (S) int32 GPU tensor or None.  Returns a dict of int64 GPU tensors -- focal,
    pairs, overlap (S, K+1), ttc (S, K+1, tau_bins), dist (S, K+1, r_bins), nn (S, r_bins+1), min_ttc (S, tau_bins+1) --
    with no host synchronisation (capturable in a graph)."""
    import ctypes
    (P, V, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, V=V, M=M), frames, n_active)
    lags = [int(x) for x in lags]
    K, TB, RB = len(lags), int(tau_bins), int(r_bins)
    x0, x1, y0, y1 = (0.0, 0.0, 0.0, 0.0) if box is None else (float(v) for v in box)
    i64 = dict(device=dev, dtype=torch.int64)
    K1, TBc, RBc = K + 1, max(TB, 0), max(RB, 0)
    out = dict(focal=torch.empty(S, K1, **i64), pairs=torch.empty(S, K1, **i64), overlap=torch.empty(S, K1, **i64),
               ttc=torch.empty(S, K1, TBc, **i64), dist=torch.empty(S, K1, RBc, **i64), nn=torch.empty(S, RBc + 1, **i64),
               min_ttc=torch.empty(S, TBc + 1, **i64))
    L = _lib.lib()
    _, ws = _stats_new(False, dev, L.piml_pair_stats_workspace_bytes(S, K, TBc, RBc))
    lag_arr = (ctypes.c_int * max(K, 1))(*lags)
    with torch.cuda.device(dev):
        _lib.check(L.piml_pair_stats(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), S, T, N, a, b,
                                     ctypes.addressof(lag_arr) if K else None, K, float(radius),
                                     float(r_max) if r_max is not None else 0.0, int(box is not None), x0, x1, y0, y1,
                                     float(tau_bin), TB, float(r_bin), RB, _ptr(out['focal']), _ptr(out['pairs']),
                                     _ptr(out['overlap']), _ptr(out['ttc']), _ptr(out['dist']), _ptr(out['nn']),
                                     _ptr(out['min_ttc']), _ptr(ws), ws.numel(), _stream()),
                   'piml_pair_stats')
    return out


FLOW_MAX_BINS = 256           # piml_flow_stats' limits on r_bins and the slots per frame
FLOW_MAX_N = 65536
FLOW_Q = 1 << 20              # the fixed-point scale of corr_sum, lane_sum, map_vx and map_vy
FLOW_SERIES = ('lane_n', 'lane_sum', 'lane_same', 'lane_opp', 'dir_plus', 'dir_minus')


def flow_stats_frames(P, V, M, v_min=0.1, r_bin=0.1, r_bins=60, r_max=6.0, axis=(1.0, 0.0), lane_width=0.5,
                      lane_length=5.0, box=None, grid=None, cell=0.5, frames=None, n_active=None):
    """The device half of piml_amd.flowstats.flow_stats (piml_flow_stats): P, V (S, T, N, 2) and M (S, T, N)
    float32 GPU tensors, axis a unit 2-vector, box (x0, x1, y0, y1) with its grid (gx, gy) or None, frames (a, b) or None,
    n_active (S) int32 GPU tensor or None.  Returns a dict of int64 GPU tensors -- corr_pairs, corr_sum (S, r_bins);
    lane_n, lane_sum, lane_same, lane_opp, dir_plus, dir_minus (S, T'); map_n, map_vx, map_vy (S, gy, gx) or None -- with
    no host synchronisation (capturable in a graph)."""
    (P, V, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, V=V, M=M), frames, n_active)
    RB, Tp = int(r_bins), max(b - a, 0)
    gx, gy = (0, 0) if box is None else (int(grid[0]), int(grid[1]))
    rect = (0.0, 0.0, 0.0, 0.0) if box is None else tuple(float(v) for v in box)
    L = _lib.lib()
    new, ws = _stats_new(S * Tp * N == 0, dev, L.piml_flow_stats_workspace_bytes(S, max(RB, 0), max(gx, 0), max(gy, 0)))
    i64 = dict(device=dev, dtype=torch.int64)
    out = {k: new(S, max(RB, 0), **i64) for k in ('corr_pairs', 'corr_sum')}
    out.update({k: new(S, Tp, **i64) for k in FLOW_SERIES})
    out.update({k: new(S, gy, gx, **i64) if box is not None else None for k in ('map_n', 'map_vx', 'map_vy')})
    with torch.cuda.device(dev):
        _lib.check(L.piml_flow_stats(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), S, T, N, a, b, float(v_min), float(r_bin),
                                     RB, float(r_max), float(axis[0]), float(axis[1]), float(lane_width),
                                     float(lane_length), int(box is not None), *rect, float(cell), gx, gy,
                                     *(_ptr(out[k]) for k in ('corr_pairs', 'corr_sum') + FLOW_SERIES
                                       + ('map_n', 'map_vx', 'map_vy')), _ptr(ws), ws.numel(), _stream()),
                   'piml_flow_stats')
    return out


VIEW_MAX_HALF = 16            # piml_view_stats' limits on half (the map is 2 half x 2 half), gap_bins, the number of lags
VIEW_MAX_BINS = 256           # and the slots per frame
VIEW_MAX_LAGS = 8
VIEW_MAX_N = 65536
VIEW_Q = 1 << 20              # the fixed-point scale of front_speed
VIEW_COS_SAME = float(np.float32(np.cos(np.pi / 4)))


def view_stats_frames(P, V, M, lags=(64, 128, 192), v_min=0.1, cell=0.25, half=12, cos_same=VIEW_COS_SAME, r_max=None,
                      corridor=0.4, gap_bin=0.1, gap_bins=60, box=None, frames=None, n_active=None):
    """The device half of piml_amd.viewstats.view_stats (piml_view_stats): P, V (S, T, N, 2) and M (S, T, N)
    float32 GPU tensors, lags a sequence of K positive ascending ints, r_max a distance or None, box (x0, x1, y0, y1) or
    None, frames (a, b) or None, n_active (S) int32 GPU tensor or None.  Returns a dict of int64 GPU tensors -- focal, pairs
    (S, K+1), map (S, K+1, 4, G, G) with G = 2 half, nn_map (S, G G + 1), front_gap (S, gap_bins+1), front_speed (S,
    gap_bins) -- with no host synchronisation (capturable in a graph)."""
    import ctypes
    (P, V, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, V=V, M=M), frames, n_active)
    lags = [int(x) for x in lags]
    K, H, GB = len(lags), int(half), int(gap_bins)
    x0, x1, y0, y1 = (0.0, 0.0, 0.0, 0.0) if box is None else (float(v) for v in box)
    i64 = dict(device=dev, dtype=torch.int64)
    K1, G, GBc = K + 1, 2 * max(H, 0), max(GB, 0)
    out = dict(focal=torch.empty(S, K1, **i64), pairs=torch.empty(S, K1, **i64), map=torch.empty(S, K1, 4, G, G, **i64),
               nn_map=torch.empty(S, G * G + 1, **i64), front_gap=torch.empty(S, GBc + 1, **i64),
               front_speed=torch.empty(S, GBc, **i64))
    L = _lib.lib()
    _, ws = _stats_new(False, dev, L.piml_view_stats_workspace_bytes(S, K, max(H, 0), GBc))
    lag_arr = (ctypes.c_int * max(K, 1))(*lags)
    with torch.cuda.device(dev):
        _lib.check(L.piml_view_stats(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), S, T, N, a, b,
                                     ctypes.addressof(lag_arr) if K else None, K, float(v_min), float(cell), H,
                                     float(cos_same), float(r_max) if r_max is not None else 0.0, float(corridor),
                                     float(gap_bin), GB, int(box is not None), x0, x1, y0, y1,
                                     *(_ptr(out[k]) for k in ('focal', 'pairs', 'map', 'nn_map', 'front_gap', 'front_speed')),
                                     _ptr(ws), ws.numel(), _stream()),
                   'piml_view_stats')
    return out


TRACK_TILE = 1024             # piml_track_stats: frames per staged LDS tile (PIML_TRACK_TILE), lags per pass
TRACK_LAG_LANES = 128         # (PIML_TRACK_LAG_LANES), and its limits on n_lags, the slots per frame, acc_bins and d_max
TRACK_MAX_LAGS = 512
TRACK_MAX_N = 65536
TRACK_MAX_BINS = 256
TRACK_MAX_D = 1024.0
TRACK_MAX_FRAMES = 1 << 25   # frames per window: a track's path sum stays below 2^63
TRACK_Q = 1 << 20             # the fixed-point scale of ac_sum, msd_sum, acc_sum, trk_path and trk_net
TRACK_LAG_ROWS = ('ac_n', 'ac_sum', 'msd_n', 'msd_sum', 'msd_far')
TRACK_ROWS = ('trk_frames', 'trk_steps', 'trk_first', 'trk_last', 'trk_path', 'trk_net')


def track_stats_frames(P, M, dt=0.08, v_min=0.1, n_lags=128, d_max=64.0, acc_bin=0.25, acc_bins=40, frames=None,
                       n_active=None):
    """The device half of piml_amd.trackstats.track_stats (piml_track_stats): P (S, T, N, 2) and M (S, T, N)
    float32 GPU tensors, frames (a, b) or None, n_active (S) int32 GPU tensor or None.  Returns a dict of int64 GPU tensors --
    ac_n, ac_sum, msd_n, msd_sum, msd_far (S, n_lags); acc (S, acc_bins + 1); acc_sum (S); trk_frames, trk_steps, trk_first,
    trk_last, trk_path, trk_net (S, N) -- with no host synchronisation (capturable in a graph)."""
    (P, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, M=M), frames, n_active)
    NL, AB, Tp = int(n_lags), int(acc_bins), max(b - a, 0)
    L = _lib.lib()
    idle = S * Tp * N == 0                    # then the outputs get the values of empty tracks
    new, ws = _stats_new(idle, dev, L.piml_track_stats_workspace_bytes(S, max(NL, 0), max(AB, 0)))
    i64 = dict(device=dev, dtype=torch.int64)
    out = {k: new(S, max(NL, 0), **i64) for k in TRACK_LAG_ROWS}
    out['acc'] = new(S, max(AB, 0) + 1, **i64)
    out['acc_sum'] = new(S, **i64)
    out.update({k: new(S, N, **i64) for k in TRACK_ROWS})
    if idle:
        out['trk_first'] -= 1
        out['trk_last'] -= 1
    with torch.cuda.device(dev):
        _lib.check(L.piml_track_stats(_ptr(P), _ptr(M), _ptr(n_active), S, T, N, a, b, float(dt), float(v_min), NL,
                                      float(d_max), float(acc_bin), AB,
                                      *(_ptr(out[k]) for k in TRACK_LAG_ROWS + ('acc', 'acc_sum') + TRACK_ROWS), _ptr(ws),
                                      ws.numel(), _stream()),
                   'piml_track_stats')
    return out


OBS_TILE = 4096               # piml_obstacle_stats: obstacle points per staged LDS tile (PIML_OBS_TILE), and its limits on the
OBS_MAX_N = 65536             # slots per frame, the obstacle points and r_bins / tau_bins
OBS_MAX_O = 1 << 24
OBS_MAX_BINS = 256
OBS_Q = 1 << 20               # the fixed-point scale of clear_speed, clear_sum and trk_min
OBS_COUNTS = ('focal', 'steps', 'contact', 'hit', 'clear_sum')
OBS_R_ROWS = ('clear', 'clear_speed', 'swept')
OBS_TRACK_ROWS = ('trk_frames', 'trk_contacts', 'trk_hits', 'trk_min')


def obstacle_stats_frames(P, V, M, obstacles, dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.05, r_bins=100, tau_bin=0.1,
                          tau_bins=100, box=None, frames=None, n_active=None):
    """The device half of piml_amd.obstaclestats.obstacle_stats (piml_obstacle_stats): P, V (S, T, N, 2), M
    (S, T, N) and obstacles (O, 2) float32 GPU tensors, box (x0, x1, y0, y1) or None, frames (a, b) or None, n_active (S)
    int32 GPU tensor or None.  Returns a dict of int64 GPU tensors -- focal, steps, contact, hit, clear_sum (S); clear,
    clear_speed, swept (S, r_bins + 1); min_ttc (S, tau_bins + 1); trk_frames, trk_contacts, trk_hits, trk_min (S, N) -- with
    no host synchronisation (capturable in a graph)."""
    (P, V, M, obstacles), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, V=V, M=M, obstacles=obstacles), frames,
                                                                        n_active)
    if obstacles.dim() != 2 or obstacles.shape[-1] != 2:
        raise ValueError(f'obstacles: expected (O, 2), got {tuple(obstacles.shape)}')
    O = obstacles.shape[0]
    RB, TB, Tp = int(r_bins), int(tau_bins), max(b - a, 0)
    x0, x1, y0, y1 = (0.0, 0.0, 0.0, 0.0) if box is None else (float(v) for v in box)
    L = _lib.lib()
    idle = S * Tp * N * O == 0                # then the outputs get the values of an empty problem
    new, ws = _stats_new(idle, dev, L.piml_obstacle_stats_workspace_bytes(S, N, max(RB, 0), max(TB, 0)))
    i64 = dict(device=dev, dtype=torch.int64)
    out = {k: new(S, **i64) for k in OBS_COUNTS}
    out.update({k: new(S, max(RB, 0) + 1, **i64) for k in OBS_R_ROWS})
    out['min_ttc'] = new(S, max(TB, 0) + 1, **i64)
    out.update({k: new(S, N, **i64) for k in OBS_TRACK_ROWS})
    if idle:
        out['trk_min'] -= 1
    with torch.cuda.device(dev):
        _lib.check(L.piml_obstacle_stats(_ptr(P), _ptr(V), _ptr(M), _ptr(n_active), S, T, N, a, b, _ptr(obstacles), O,
                                         float(dt), float(radius), float(hit_radius), int(box is not None), x0, x1, y0, y1,
                                         float(r_bin), RB, float(tau_bin), TB,
                                         *(_ptr(out[k]) for k in OBS_COUNTS[:4]), _ptr(out['clear_sum']),
                                         *(_ptr(out[k]) for k in OBS_R_ROWS), _ptr(out['min_ttc']),
                                         *(_ptr(out[k]) for k in OBS_TRACK_ROWS), _ptr(ws), ws.numel(), _stream()),
                   'piml_obstacle_stats')
    return out


LINE_MAX_L = 16               # piml_line_stats: its limits on the lines (PIML_LINE_MAX_L), the slots per frame, v_bins /
LINE_MAX_N = 65536            # w_bins and the frames per window, and the steps a lane sweeps per work item
LINE_MAX_BINS = 256
LINE_MAX_FRAMES = 1 << 25
LINE_CHUNK = 32
LINE_Q = 1 << 20              # the fixed-point scale of speed_sum and of the crossing times trk_first
LINE_DIR_ROWS = ('cross', 'speed_sum')
LINE_TRACK_ROWS = ('trk_count', 'trk_first', 'trk_dir')
LINE_ROWS = ('cross', 'nt', 'speed', 'speed_sum', 'profile', 'steps', 'trk_steps') + LINE_TRACK_ROWS


def line_stats_frames(P, M, lines, dt=0.08, v_bin=0.1, v_bins=40, w_bins=16, frames=None, n_active=None):
    """The device half of piml_amd.linestats.line_stats (piml_line_stats): P (S, T, N, 2), M (S, T, N) and
    lines (L, 4) float32 GPU tensors (rows ax, ay, bx, by; their values are the caller's to check: a bad row counts no
    crossing), frames (a, b) or None, n_active (S) int32 GPU tensor or None.  Returns a dict of int64 GPU tensors -- cross,
    speed_sum (S, L, 2); nt (S, L, 2, T'); speed (S, L, 2, v_bins + 1); profile (S, L, 2, w_bins); steps (S); trk_steps (S, N);
    trk_count, trk_first, trk_dir (S, L, N) -- with no host synchronisation (capturable in a graph)."""
    (P, M, lines), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, M=M, lines=lines), frames, n_active)
    if lines.dim() != 2 or lines.shape[-1] != 4:
        raise ValueError(f'lines: expected (L, 4), got {tuple(lines.shape)}')
    NL = lines.shape[0]
    VB, WB, Tp = int(v_bins), int(w_bins), max(b - a, 0)
    L = _lib.lib()
    idle = S * Tp * N * NL == 0               # then the outputs get the values of an empty problem
    new, ws = _stats_new(idle, dev, L.piml_line_stats_workspace_bytes(S, N, NL, Tp, max(VB, 0), max(WB, 0)))
    i64 = dict(device=dev, dtype=torch.int64)
    out = {k: new(S, NL, 2, **i64) for k in LINE_DIR_ROWS}
    out['nt'] = new(S, NL, 2, Tp, **i64)
    out['speed'] = new(S, NL, 2, max(VB, 0) + 1, **i64)
    out['profile'] = new(S, NL, 2, max(WB, 0), **i64)
    out['steps'] = new(S, **i64)
    out['trk_steps'] = new(S, N, **i64)
    out.update({k: new(S, NL, N, **i64) for k in LINE_TRACK_ROWS})
    if idle:
        out['trk_first'] -= 1
        out['trk_dir'] -= 1
    with torch.cuda.device(dev):
        _lib.check(L.piml_line_stats(_ptr(P), _ptr(M), _ptr(n_active), S, T, N, a, b, _ptr(lines), NL, float(dt),
                                     float(v_bin), VB, WB, *(_ptr(out[k]) for k in LINE_ROWS), _ptr(ws), ws.numel(),
                                     _stream()),
                   'piml_line_stats')
    return out


GROUP_MAX_N = 65536           # piml_group_pairs / piml_group_members: their limits on the slots per frame, the frames per
GROUP_MAX_FRAMES = 1 << 25    # window, r_bins / a_bins and the default cap on the edge rows per member, the focal frames
GROUP_MAX_BINS = 256          # staged per LDS tile, the fixed-point scale of trk_path and dist_sum, the unit of `share`
GROUP_MAX_EDGES = 1 << 20
GROUP_TILE = 256
GROUP_Q = 1 << 20
GROUP_SHARE_UNIT = 1024
GROUP_PAIR_ROWS = ('trk_steps', 'trk_path', 'pairs', 'together')
GROUP_MEMBER_ROWS = ('dist', 'dist_sum', 'abreast', 'abreast_skipped', 'link_frames')


def group_thresholds(dt, radius, dv_max, v_min, min_time, share):
    """What the kernels and a restatement receive: (r2, dv2, vm2) = float32 of radius^2, (dv_max dt)^2, (v_min dt)^2, each made
    once in float64 and rounded once; min_frames = max(1, ceil(min_time / dt)); share_q = round(share * 1024)."""
    dt, radius, dv_max, v_min = float(dt), float(radius), float(dv_max), float(v_min)
    r2, dv2, vm2 = (float(np.float32(x)) for x in (radius * radius, (dv_max * dt) ** 2, (v_min * dt) ** 2))
    return r2, dv2, vm2, max(1, math.ceil(float(min_time) / dt)), int(round(float(share) * GROUP_SHARE_UNIT))


def group_pairs_frames(P, M, r2, dv2, vm2, min_frames, frames=None, n_active=None, max_edges=None):
    """Pass 1 of the group statistics alone (piml_group_pairs): P (S, T, N, 2), M (S, T, N) float32 GPU tensors,
    the thresholds of group_thresholds, frames (a, b) or None, n_active (S) int32 GPU tensor or None; max_edges None:
    min(N (N - 1) / 2, 2^20).  Returns a dict of GPU tensors -- edges (S, max_edges, 4) int32, rows (i, j, co, near) of the
    candidates in any order (rows at or past n_edges[s] hold nothing), n_edges (S) int32 the true count, trk_steps, trk_path
    (S, N) and pairs, together (S) int64 -- with no host synchronisation (capturable in a graph)."""
    (P, M), (S, T, N, a, b), dev, n_active = _stats_setup(dict(P=P, M=M), frames, n_active)
    cap = min(N * (N - 1) // 2, GROUP_MAX_EDGES) if max_edges is None else int(max_edges)
    new, _ = _stats_new(S * max(b - a, 0) * N == 0, dev)
    out = {'edges': new(S, max(cap, 0), 4, device=dev, dtype=torch.int32), 'n_edges': new(S, device=dev, dtype=torch.int32),
           'trk_steps': new(S, N, device=dev, dtype=torch.int64), 'trk_path': new(S, N, device=dev, dtype=torch.int64),
           'pairs': new(S, device=dev, dtype=torch.int64), 'together': new(S, device=dev, dtype=torch.int64)}
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().piml_group_pairs(_ptr(P), _ptr(M), _ptr(n_active), S, T, N, a, b, float(r2), float(dv2), float(vm2),
                                               int(min_frames), cap, _ptr(out['edges']) if cap > 0 else None,
                                               _ptr(out['n_edges']), *(_ptr(out[k]) for k in GROUP_PAIR_ROWS), _stream()),
                   'piml_group_pairs')
    return out


def group_members_frames(P, M, links, r2, dv2, vm2, r_bin=0.1, r_bins=20, a_bins=10, frames=None):
    """Pass 2 of the group statistics alone (piml_group_members): links (K, 3) int32 GPU tensor, rows (member, i, j).  Returns
    a dict of int64 GPU tensors -- dist (S, r_bins + 1), abreast (S, a_bins), dist_sum, abreast_skipped, link_frames (S)."""
    (P, M), (S, T, N, a, b), dev, _ = _stats_setup(dict(P=P, M=M), frames, None)
    if not isinstance(links, torch.Tensor) or links.device != dev or links.dtype != torch.int32 or links.dim() != 2 \
            or links.shape[1] != 3:
        raise ValueError(f'links: expected an int32 (K, 3) tensor on {dev}')
    links = links.contiguous()
    RB, AB = int(r_bins), int(a_bins)
    i64 = dict(device=dev, dtype=torch.int64)
    out = {'dist': torch.zeros(S, max(RB, 0) + 1, **i64), 'dist_sum': torch.zeros(S, **i64),
           'abreast': torch.zeros(S, max(AB, 0), **i64), 'abreast_skipped': torch.zeros(S, **i64),
           'link_frames': torch.zeros(S, **i64)}
    K = links.shape[0]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().piml_group_members(_ptr(P), _ptr(M), S, T, N, a, b, _ptr(links) if K else None, K, float(r2),
                                                 float(dv2), float(vm2), float(r_bin), RB, AB,
                                                 *(_ptr(out[k]) for k in GROUP_MEMBER_ROWS), _stream()),
                   'piml_group_members')
    return out


GROUP_MAX_G = 64               # piml_group_components: the largest g_max
GROUP_COMPONENT_ROWS = ('candidates', 'links', 'group_id', 'size_tracks', 'size_path', 'size_steps')


def group_components_frames(edges, n_edges, trk_steps, trk_path, min_frames, share_q, g_max=8):
    """The host half of the group statistics on the device (piml_group_components): edges (S, cap, 4) int32,
    rows (i, j, co, near) in any order, n_edges (S) int32, trk_steps, trk_path (S, N) int64 GPU tensors -- what
    group_pairs_frames returns, unsorted.  Returns a dict of GPU tensors, piml_amd.groupstats.host_rows' bit for bit:
    candidates, links (S) int64, group_id (S, N) int32, size_tracks, size_path, size_steps (S, g_max + 1) int64, and status
    (S) int32 (0; non-zero only if the kernel's rounds did not settle, a defect).  One launch that writes every element, no
    host synchronisation (capturable in a graph)."""
    for name, x, dt, nd in (('edges', edges, torch.int32, 3), ('n_edges', n_edges, torch.int32, 1),
                            ('trk_steps', trk_steps, torch.int64, 2), ('trk_path', trk_path, torch.int64, 2)):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.PimlHipError(f'{name}: a GPU tensor expected')
        if x.dtype != dt or x.dim() != nd:
            raise ValueError(f'{name}: expected a {nd}-dimensional {dt} tensor, got {tuple(x.shape)} {x.dtype}')
    dev = trk_steps.device
    S, N = trk_steps.shape
    if edges.shape[0] != S or edges.shape[2] != 4 or tuple(n_edges.shape) != (S,) or tuple(trk_path.shape) != (S, N) \
            or any(x.device != dev for x in (edges, n_edges, trk_path)):
        raise ValueError(f'expected edges ({S}, cap, 4), n_edges ({S},) and trk_path ({S}, {N}) on {dev}, got '
                         f'{tuple(edges.shape)}, {tuple(n_edges.shape)}, {tuple(trk_path.shape)}')
    edges, n_edges, trk_steps, trk_path = (x.contiguous() for x in (edges, n_edges, trk_steps, trk_path))
    cap, G = edges.shape[1], int(g_max)
    new = torch.zeros if S * N == 0 else torch.empty
    i64, i32 = dict(device=dev, dtype=torch.int64), dict(device=dev, dtype=torch.int32)
    out = {'candidates': new(S, **i64), 'links': new(S, **i64), 'group_id': new(S, N, **i32),
           'size_tracks': new(S, max(G, 0) + 1, **i64), 'size_path': new(S, max(G, 0) + 1, **i64),
           'size_steps': new(S, max(G, 0) + 1, **i64), 'status': new(S, **i32)}
    work = torch.empty(S, N, **i32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().piml_group_components(_ptr(edges) if cap > 0 else None, _ptr(n_edges), _ptr(trk_steps),
                                                    _ptr(trk_path), S, N, cap, int(min_frames), int(share_q), G,
                                                    *(_ptr(out[k]) for k in GROUP_COMPONENT_ROWS), _ptr(work),
                                                    _ptr(out['status']), _stream()), 'piml_group_components')
    return out


def group_stats_frames(P, M, dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8, r_bin=0.1, r_bins=20,
                       a_bins=10, frames=None, n_active=None, max_edges=None, components='host', g_max=8):
    """The device half of piml_amd.groupstats.group_stats: the pair sweep, the link rule, the member
    statistics.  P (S, T, N, 2), M (S, T, N) float32 GPU tensors, frames (a, b) or None, n_active (S) int32 GPU tensor or
    None.  Returns a dict of GPU tensors: edges (E, 5) int64, rows (member, i, j, co, near) of every candidate sorted by
    (member, i, j); n_edges (S) int64; trk_steps, trk_path (S, N), pairs, together (S) int64; and the rows of
    group_members_frames over the links (near * 1024 >= round(share * 1024) * co).  The candidate counts are read back
    between the passes (not capturable; group_pairs_frames alone is).  ValueError when a member has more than max_edges
    candidates (None: min(N (N - 1) / 2, 2^20)), naming the count that was needed.  components='device' also returns the six
    rows of the host half (candidates, links, group_id, size_tracks, size_path, size_steps) and `status` as GPU
    tensors: group_components_frames on pass 1's unsorted rows, after the capacity check; 'host' (the default) leaves them to
    piml_amd.groupstats.host_rows."""
    if components not in ('host', 'device'):
        raise ValueError(f"components: 'host' or 'device' expected, got {components!r}")
    r2, dv2, vm2, min_frames, share_q = group_thresholds(dt, radius, dv_max, v_min, min_time, share)
    raw = group_pairs_frames(P, M, r2, dv2, vm2, min_frames, frames, n_active, max_edges)
    n = raw['n_edges'].to(torch.int64)
    cap = raw['edges'].shape[1]
    need = int(n.max().item()) if n.numel() else 0
    if need > cap:
        raise ValueError(f'group_stats: a member has {need} candidate pairs, max_edges is {cap}: pass max_edges={need}')
    S = n.shape[0]
    comp = None
    if components == 'device':
        comp = group_components_frames(raw['edges'], raw['n_edges'], raw['trk_steps'], raw['trk_path'], min_frames, share_q, g_max)
    rows = raw['edges'][:, :need].to(torch.int64)                                 # (S, need, 4)
    valid = torch.arange(need, device=n.device)[None, :] < n[:, None]
    member = torch.arange(S, device=n.device)[:, None].expand(S, need)
    flat = torch.cat([member[valid][:, None], rows[valid]], 1)                    # (E, 5)
    order = torch.argsort((flat[:, 0] << 32) | (flat[:, 1] << 16) | flat[:, 2]) if flat.shape[0] else flat[:, 0]
    edges = flat[order]
    link = edges[:, 4] * GROUP_SHARE_UNIT >= share_q * edges[:, 3]
    out = {'edges': edges, 'n_edges': n}
    out.update({k: raw[k] for k in GROUP_PAIR_ROWS})
    out.update(group_members_frames(P, M, edges[link][:, :3].to(torch.int32), r2, dv2, vm2, r_bin, r_bins, a_bins, frames))
    if comp is not None:
        out.update(comp)
    return out
