"""Numpy restatement of the obstacle statistics (piml_amd.obstaclestats), with the items whose classification
float32 cannot be trusted to share flagged as ambiguous.

Everything is computed twice: in float32 numpy, the formulas as written with each operation rounded (IEEE subtraction,
product, sum, division and square root are correctly rounded in numpy and on the device alike, np.fmin / np.fmax drop a NaN
as fminf / fmaxf do, and rint rounds to even as llrintf does) -- the run the device is expected to reproduce bit for bit,
since a minimum is exact whatever the order of the points -- and in float64 over the same float32 inputs and options.  An
item is a focal agent-frame (with at least one valid obstacle point).  It is ambiguous when any bin or predicate differs
between the two runs: the clearance bin, contact, r < r_bin * r_bins, the bin of the smallest time to an obstacle, and for
a step the swept-clearance bin and hit.

obstacle_stats returns the float32 run's outputs, the float64 run's (`f64`), n_items, n_ambiguous and the ambiguous items
per member (`ambiguous`).  check() demands device == float32 run for every member without an ambiguous item, and for the
others every count and histogram entry within the member's number of ambiguous items of it."""
import numpy as np

COUNTS = ('focal', 'steps', 'contact', 'hit', 'clear_sum')
R_ROWS = ('clear', 'clear_speed', 'swept')
TRACK_ROWS = ('trk_frames', 'trk_contacts', 'trk_hits', 'trk_min')
OUTPUTS = COUNTS + R_ROWS + ('min_ttc',) + TRACK_ROWS
SUMS = ('clear_sum', 'clear_speed', 'trk_min')          # fixed-point sums and values: not bounded by a count of items
HISTS = ('trk_min_hist', 'tracks', 'tracks_hit', 'tracks_contact')
Q = 1 << 20
MAX_COORD = 65536.0
MAX_SPEED = 1024.0
MAX_R = 16777216.0
PREDICATES = ('rb', 'contact', 'summed', 'tb', 'sb', 'hit')


def participants(p, v, m):
    with np.errstate(invalid='ignore'):
        return (m == 1) & (np.abs(p) < MAX_COORD).all(-1) & (np.abs(v) < MAX_SPEED).all(-1)


def _rint(x):
    return np.rint(np.where(np.isfinite(x), x, 0)).astype(np.int64)


def _bin(x, width, bins):
    with np.errstate(all='ignore'):
        q = np.floor(x / width)
        return np.where(q < bins, q, bins).astype(np.int64)


def _items(p, v, p1, step, pts, o, dt, chunk=1 << 16):
    """every per-item quantity in dtype dt: p, v (n, 2) float32, p1 (n, 2) the position a frame later where `step` (n) says
    the step exists, pts (k, 2) float32 valid points"""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    radius, hit_radius, r_bin, tau_bin = f(o['radius']), f(o['hit_radius']), f(o['r_bin']), f(o['tau_bin'])
    RB, TB = o['r_bins'], o['tau_bins']
    r2, r_top = radius * radius, r_bin * dt(RB)
    n, k = p.shape[0], pts.shape[0]
    p, v, q = p.astype(dt), v.astype(dt), pts.astype(dt)
    with np.errstate(all='ignore'):
        u = np.where(step[:, None], p1.astype(dt) - p, 0).astype(dt)
    min_d2, min_m2, min_tau = (np.full(n, np.inf, dt) for _ in range(3))
    rows = max(1, chunk // max(k, 1))
    with np.errstate(all='ignore'):
        aa = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
        len2 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
        for lo in range(0, n, rows):
            sl = slice(lo, lo + rows)
            ex = q[None, :, 0] - p[sl, None, 0]
            ey = q[None, :, 1] - p[sl, None, 1]
            d2 = ex * ex + ey * ey
            min_d2[sl] = np.fmin.reduce(d2, axis=1, initial=np.inf)
            ux, uy, l2 = u[sl, None, 0], u[sl, None, 1], len2[sl, None]
            s = np.where(l2 != 0, np.fmin(np.fmax((ex * ux + ey * uy) / np.where(l2 != 0, l2, 1), 0), 1), 0).astype(dt)
            fx, fy = ex - s * ux, ey - s * uy
            min_m2[sl] = np.fmin.reduce(fx * fx + fy * fy, axis=1, initial=np.inf)
            c = d2 - r2
            b = -(ex * v[sl, None, 0] + ey * v[sl, None, 1])
            disc = b * b - aa[sl, None] * c
            course = (c >= 0) & (b < 0) & (disc >= 0)
            tau = np.where(course, c / (-b + np.sqrt(np.where(course, disc, 0))), np.inf).astype(dt)
            min_tau[sl] = np.fmin.reduce(tau, axis=1, initial=np.inf)
        rr, m = np.sqrt(min_d2), np.sqrt(min_m2)
        res = dict(rb=_bin(rr, r_bin, RB), contact=rr < radius, summed=rr < r_top, tb=_bin(min_tau, tau_bin, TB),
                   sb=np.where(step, _bin(m, r_bin, RB), -1), hit=step & (m < hit_radius),
                   rq=_rint(rr * dt(Q)), speed_q=_rint(np.sqrt(aa) * dt(Q)), min_q=_rint(np.fmin(rr, dt(MAX_R)) * dt(Q)))
    return res


def obstacle_stats(P, V, M, obs, dt=0.08, radius=0.25, hit_radius=0.1, r_bin=0.05, r_bins=100, tau_bin=0.1, tau_bins=100,
                   box=None, frames=None, n_active=None):
    P, V, M = np.asarray(P, np.float32), np.asarray(V, np.float32), np.asarray(M, np.float32)
    if P.ndim == 3:
        P, V, M = P[None], V[None], M[None]
    obs = np.asarray(obs, np.float32).reshape(-1, 2)
    S, T, N = M.shape
    t0, t1 = frames if frames is not None else (0, T)
    Tp, RB, TB = t1 - t0, int(r_bins), int(tau_bins)
    o = dict(radius=radius, hit_radius=hit_radius, r_bin=r_bin, r_bins=RB, tau_bin=tau_bin, tau_bins=TB)
    z = lambda *shape: np.zeros(shape, np.int64)

    def blank():
        d = {k: z(S) for k in COUNTS}
        d.update({k: z(S, RB + 1) for k in R_ROWS})
        d['min_ttc'] = z(S, TB + 1)
        d.update({k: z(S, N) for k in TRACK_ROWS})
        d['trk_min'] -= 1
        return d
    out, f64 = blank(), blank()
    amb = z(S)
    n_items = 0
    pts = obs[np.isfinite(obs).all(1)]
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        if bound == 0 or Tp == 0 or obs.shape[0] == 0:
            continue
        p, v, m = P[s, t0:t1, :bound], V[s, t0:t1, :bound], M[s, t0:t1, :bound]
        part = participants(p, v, m)
        focal = part
        if box is not None:
            x0, x1, y0, y1 = (np.float32(b) for b in box)
            with np.errstate(invalid='ignore'):
                focal = part & (x0 <= p[..., 0]) & (p[..., 0] < x1) & (y0 <= p[..., 1]) & (p[..., 1] < y1)
        step = np.zeros_like(focal)
        step[:-1] = focal[:-1] & part[1:]
        t_idx, i_idx = np.nonzero(focal)
        ip, iv, istep = p[t_idx, i_idx], v[t_idx, i_idx], step[t_idx, i_idx]
        ip1 = p[np.minimum(t_idx + 1, Tp - 1), i_idx]
        for dst in (out, f64):
            dst['focal'][s], dst['steps'][s] = int(focal.sum()), int(step.sum())
        if pts.shape[0] == 0:
            continue
        runs = [_items(ip, iv, ip1, istep, pts, o, d) for d in (np.float32, np.float64)]
        for res, dst in zip(runs, (out, f64)):
            dst['contact'][s], dst['hit'][s] = int(res['contact'].sum()), int(res['hit'].sum())
            dst['clear_sum'][s] = int(res['rq'][res['summed']].sum())
            np.add.at(dst['clear'][s], res['rb'], 1)
            np.add.at(dst['clear_speed'][s], res['rb'], res['speed_q'])
            np.add.at(dst['swept'][s], res['sb'][istep], 1)
            np.add.at(dst['min_ttc'][s], res['tb'], 1)
            np.add.at(dst['trk_frames'][s], i_idx, 1)
            np.add.at(dst['trk_contacts'][s], i_idx, res['contact'].astype(np.int64))
            np.add.at(dst['trk_hits'][s], i_idx, res['hit'].astype(np.int64))
            low = np.full(N, np.iinfo(np.int64).max)
            np.minimum.at(low, i_idx, res['min_q'])
            dst['trk_min'][s] = np.where(dst['trk_frames'][s] > 0, low, -1)
        differs = np.zeros(len(t_idx), bool)
        for k in PREDICATES:
            differs |= runs[0][k] != runs[1][k]
        amb[s] = int(differs.sum())
        n_items += len(t_idx)
    out['f64'], out['ambiguous'] = f64, amb
    out['n_items'], out['n_ambiguous'] = n_items, int(amb.sum())
    return out


def host_rows(rows, r_bin, r_bins):
    """the host half, one track at a time: trk_min_hist (S, r_bins + 1), tracks, tracks_hit, tracks_contact (S)"""
    fr, co, hi, mn = (np.asarray(rows[k]) for k in TRACK_ROWS)
    S, N = fr.shape
    width = float(np.float32(r_bin))
    out = dict(trk_min_hist=np.zeros((S, r_bins + 1), np.int64), tracks=np.zeros(S, np.int64), tracks_hit=np.zeros(S, np.int64),
               tracks_contact=np.zeros(S, np.int64))
    for s in range(S):
        for n in range(N):
            if fr[s, n] <= 0:
                continue
            out['tracks'][s] += 1
            out['tracks_hit'][s] += int(hi[s, n] > 0)
            out['tracks_contact'][s] += int(co[s, n] > 0)
            out['trk_min_hist'][s, min(int(np.floor(int(mn[s, n]) / Q / width)), r_bins)] += 1
    return out


def check(got, want, label=''):
    """every device output of `got` (dict or object of int arrays) equals want's (the float32 run's) for the members without
    an ambiguous item; for the others the counts and histogram entries lie within the member's number of ambiguous items.
    Returns the largest deviation per output as (against the float32 run, against the float64 run)."""
    get = lambda k: np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
    dev = {}
    for k in OUTPUTS:
        g = get(k)
        assert g.shape == want[k].shape, (label, k, g.shape, want[k].shape)
        dev[k] = (int(np.abs(g - want[k]).max(initial=0)), int(np.abs(g - want['f64'][k]).max(initial=0)))
    print(f'[obstaclestats] {label}: largest deviation (float32 run, float64 run) ' + ', '.join(f'{k} {v}' for k, v in dev.items()))
    for k in OUTPUTS:
        g = get(k)
        for s, n_amb in enumerate(want['ambiguous'].tolist()):
            if n_amb == 0:
                assert np.array_equal(g[s], want[k][s]), (label, k, s, 'differs from the float32 run')
            elif k not in SUMS:
                assert np.abs(g[s] - want[k][s]).max(initial=0) <= n_amb, (label, k, s, n_amb)
    return dev


def random_obstacles(O, side, seed, bad=0.0):
    """O points inside a square of the given side: up to 100 on a circle of radius 1 about its centre, the rest on wall rows
    of 800 points each (spacing side / 800) taken in a scattered order so that a short list is spread over the row; a share
    `bad` of them NaN or infinite."""
    rng = np.random.default_rng(seed)
    k = np.arange(O)
    n_circle = min(O // 8, 100)
    wall = k[n_circle:] - n_circle
    pts = np.zeros((O, 2))
    ang = 2 * np.pi * k[:n_circle] / max(n_circle, 1)
    pts[:n_circle] = 0.5 * side + np.stack([np.cos(ang), np.sin(ang)], -1)
    pts[n_circle:, 0] = ((wall * 37) % 800 + 0.5) * side / 800.0
    pts[n_circle:, 1] = side * (0.2 + 0.11 * (wall // 800))
    pts = pts.astype(np.float32)
    r = rng.random(O)
    pts[r < 0.5 * bad, 0] = np.nan
    pts[(r >= 0.5 * bad) & (r < bad), 1] = np.inf
    return pts


def analytic_scene():
    """Five agents over two frames beside a wall of 129 points on y = 0 at 0.0625 spacing (x = -4 .. 4), every number
    dyadic so that each quantity is exact in float32: a tunnelling agent stepping from (0, -0.5) to (0, 0.5); one walking
    parallel to the wall at y = 0.5; a head-on approach from 1.25 m at 1 m/s (tau_min = 1.0: c = 1.5, b = -1.25,
    disc = 0.0625; a frame later from 1.125 m, tau_min = 0.875); a standing agent (len2 == 0, no tau); one walking away
    (b > 0).  Returns P, V (1, 2, 5, 2), M (1, 2, 5), obs (129, 2), the options and the hand counts."""
    obs = np.stack([np.arange(-64, 65) / 16.0, np.zeros(129)], -1).astype(np.float32)
    p0 = [(0.0, -0.5), (-1.0, 0.5), (2.0, 1.25), (-2.0, 0.75), (3.0, 0.5)]
    p1 = [(0.0, 0.5), (-0.875, 0.5), (2.0, 1.125), (-2.0, 0.75), (3.0, 0.625)]
    vel = [(0.0, 8.0), (1.0, 0.0), (0.0, -1.0), (0.0, 0.0), (0.0, 1.0)]
    P = np.array([[p0, p1]], np.float32)
    V = np.array([[vel, vel]], np.float32)
    M = np.ones((1, 2, 5), np.float32)
    kw = dict(radius=0.25, hit_radius=0.125, r_bin=0.125, r_bins=16, tau_bin=0.25, tau_bins=16)
    row = lambda n, d: [d.get(k, 0) for k in range(n)]
    hand = dict(focal=[10], steps=[5], contact=[0], hit=[1], clear_sum=[7 * Q],
                clear=[row(17, {4: 5, 5: 1, 6: 2, 9: 1, 10: 1})],
                clear_speed=[row(17, {4: 19 * Q, 5: Q, 9: Q, 10: Q})],
                swept=[row(17, {0: 1, 4: 2, 6: 1, 9: 1})],
                min_ttc=[row(17, {0: 1, 3: 1, 4: 1, 16: 7})],
                trk_frames=[[2] * 5], trk_contacts=[[0] * 5], trk_hits=[[1, 0, 0, 0, 0]],
                trk_min=[[Q // 2, Q // 2, 9 * Q // 8, 3 * Q // 4, Q // 2]],
                trk_min_hist=[row(17, {4: 3, 6: 1, 9: 1})], tracks=[5], tracks_hit=[1], tracks_contact=[0])
    return P, V, M, obs, kw, {k: np.asarray(v, np.int64) for k, v in hand.items()}
