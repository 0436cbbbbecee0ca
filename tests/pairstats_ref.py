"""Float64 numpy restatement of the pair statistics (piml_amd.pairstats), with the pairs whose classification
float32 cannot be trusted to share flagged as ambiguous.

Every pair is classified twice, in float64 (over the float32 inputs, with the float32 radius, bin widths and cut-off) and in
float32 numpy (the formulas as written, each operation rounded).  A pair is ambiguous when the two classifications differ
(evaluated, overlap, collision course, distance bin, tau bin), or when, in float64, its distance lies within
tol = max(1e-5 |x|, 1e-5) of R, of r_max or of a distance bin edge, its tau within tol of a tau bin edge, b within
max(1e-5 |d| |w|, 1e-5) of 0 or disc within max(1e-5 max(b^2, |a c|), 1e-5) of 0.  A focal agent is ambiguous for nn /
min_ttc when one of its lag-0 pairs is, or when its float32 and float64 bins differ.

pair_stats returns the float64 counts and, per output, a tolerance of the same shape: the number of ambiguous pairs (focal
agents for nn / min_ttc) that touch the bin (their float64 bin, its two neighbours and their float32 bin); for focal,
pairs and overlap the number of ambiguous pairs of the (member, lag); focal is exact."""
import numpy as np

OUTPUTS = ('focal', 'pairs', 'overlap', 'ttc', 'dist', 'nn', 'min_ttc')
REL = 1e-5


def _tol(x):
    return np.maximum(REL * np.abs(x), REL)


def participants(p, v, m):
    return (m == 1) & np.isfinite(p).all(-1) & np.isfinite(v).all(-1)


def classify(pi, vi, pj, vj, same, R, r_max, tau_bin, tau_bins, r_bin, r_bins, dt):
    """Per pair (focal rows x source columns) in dtype dt: valid, dist, dist bin (-1 when >= r_bins), overlap, course, tau
    (inf when not on a course), tau bin (-1 when none or >= tau_bins); same = the j == i slot mask."""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    R, tb, rb = f(R), f(tau_bin), f(r_bin)
    R2 = R * R
    with np.errstate(all='ignore'):
        dx = f(pj[None, :, 0]) - f(pi[:, None, 0])
        dy = f(pj[None, :, 1]) - f(pi[:, None, 1])
        wx = f(vj[None, :, 0]) - f(vi[:, None, 0])
        wy = f(vj[None, :, 1]) - f(vi[:, None, 1])
        d2 = dx * dx + dy * dy
        dist = np.sqrt(d2)
        valid = ~same
        if r_max is not None:
            valid &= ~(dist >= f(r_max))
        c = d2 - R2
        b = dx * wx + dy * wy
        a = wx * wx + wy * wy
        disc = b * b - a * c
        overlap = valid & (c < 0)
        course = valid & ~(c < 0) & (b < 0) & (disc >= 0)
        tau = np.where(course, c / (-b + np.sqrt(np.where(course, disc, 0))), np.inf).astype(dt)
        qd = np.floor(dist / rb)
        dbin = np.where(valid & (qd < r_bins), qd, -1).astype(np.int64)
        qt = np.floor(tau / tb)
        tbin = np.where(course & (qt < tau_bins), qt, -1).astype(np.int64)
    return dict(valid=valid, dist=dist, dbin=dbin, overlap=overlap, course=course, tau=tau, tbin=tbin, b=b, a=a, c=c,
                disc=disc, dnorm=np.sqrt(d2), wnorm=np.sqrt(a))


def _edge_near(x, width, nbins):
    """x within tol of a multiple k * width, k = 0 .. nbins"""
    k = np.rint(x / width)
    with np.errstate(invalid='ignore'):
        return np.isfinite(x) & (k <= nbins) & (np.abs(x - k * width) <= _tol(x))


def _min_bin(x, width, nbins):
    """bin of each row's minimum (nbins when the minimum is not below nbins * width)"""
    with np.errstate(invalid='ignore'):
        q = np.floor(x / width)
    return np.where(q < nbins, q, nbins).astype(np.int64)


def _touch(tol, b64, b32, nbins, rows=None):
    """add one to tol[rows, bin] for bin in {b64 - 1, b64, b64 + 1, b32} within [0, nbins)"""
    for b in range(len(b64)):
        touched = {b64[b] - 1, b64[b], b64[b] + 1, b32[b]}
        for x in touched:
            if 0 <= x < nbins:
                if rows is None:
                    tol[x] += 1
                else:
                    tol[rows, x] += 1


def pair_stats(P, V, M, radius=0.5, lags=(64, 128, 192), tau_bin=0.1, tau_bins=100, r_bin=0.05, r_bins=100, r_max=None,
               box=None, frames=None, n_active=None, chunk=384):
    P, V, M = (np.asarray(x, np.float32) for x in (P, V, M))
    if P.ndim == 3:
        P, V, M = P[None], V[None], M[None]
    S, T, N = M.shape
    t0, t1 = frames if frames is not None else (0, T)
    lag = [0] + [int(x) for x in lags]
    K1, TB, RB = len(lag), int(tau_bins), int(r_bins)
    bx = None if box is None else [np.float32(v) for v in box]
    R64 = np.float64(np.float32(radius))
    rmax64 = None if r_max is None else np.float64(np.float32(r_max))
    tb64, rb64 = np.float64(np.float32(tau_bin)), np.float64(np.float32(r_bin))
    z = lambda *shape: np.zeros(shape, np.int64)
    out = dict(focal=z(S, K1), pairs=z(S, K1), overlap=z(S, K1), ttc=z(S, K1, TB), dist=z(S, K1, RB), nn=z(S, RB + 1),
               min_ttc=z(S, TB + 1))
    tol = {k: np.zeros_like(v) for k, v in out.items()}
    f32 = {k: np.zeros_like(v) for k, v in out.items()}
    n_pairs = n_amb = 0
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        for k in range(K1):
            for t in range(t0, t1 - lag[k]):
                tj = t + lag[k]
                pi_, vi_, mi_ = P[s, t, :bound], V[s, t, :bound], M[s, t, :bound]
                part_i = participants(pi_, vi_, mi_)
                focal = part_i.copy()
                if bx is not None:
                    focal &= (bx[0] <= pi_[:, 0]) & (pi_[:, 0] < bx[1]) & (bx[2] <= pi_[:, 1]) & (pi_[:, 1] < bx[3])
                fi = np.nonzero(focal)[0]
                jj = np.nonzero(participants(P[s, tj, :bound], V[s, tj, :bound], M[s, tj, :bound]))[0]
                out['focal'][s, k] += len(fi)
                f32['focal'][s, k] += len(fi)
                pj, vj = P[s, tj, jj], V[s, tj, jj]
                for c0 in range(0, len(fi), chunk):
                    rows = fi[c0:c0 + chunk]
                    same = rows[:, None] == jj[None, :]
                    args = (pi_[rows], vi_[rows], pj, vj, same, radius, r_max, tau_bin, TB, r_bin, RB)
                    e, g = classify(*args, np.float64), classify(*args, np.float32)
                    # ambiguity
                    amb = np.zeros(same.shape, bool)
                    for key in ('valid', 'overlap', 'course', 'dbin', 'tbin'):
                        amb |= e[key] != g[key]
                    d = e['dist']
                    amb |= ~same & (np.abs(d - R64) <= _tol(R64))
                    if rmax64 is not None:
                        amb |= ~same & (np.abs(d - rmax64) <= _tol(rmax64))
                    v = e['valid']
                    amb |= v & _edge_near(d, rb64, RB)
                    nonov = v & ~e['overlap']
                    amb |= nonov & (np.abs(e['b']) <= np.maximum(REL * e['dnorm'] * e['wnorm'], REL))
                    near_b = nonov & (e['b'] < 0)
                    amb |= near_b & (np.abs(e['disc']) <= np.maximum(REL * np.maximum(e['b'] ** 2, np.abs(e['a'] * e['c'])),
                                                                     REL))
                    amb |= e['course'] & _edge_near(e['tau'], tb64, TB)
                    n_pairs += int(v.sum())
                    n_amb += int(amb.sum())
                    na = int(amb.sum())
                    for key in ('pairs', 'overlap'):
                        tol[key][s, k] += na
                    for res, dst in ((e, out), (g, f32)):
                        dst['pairs'][s, k] += int(res['valid'].sum())
                        dst['overlap'][s, k] += int(res['overlap'].sum())
                        db, tbn = res['dbin'], res['tbin']
                        np.add.at(dst['dist'][s, k], db[db >= 0], 1)
                        np.add.at(dst['ttc'][s, k], tbn[tbn >= 0], 1)
                    ai, aj = np.nonzero(amb)
                    _touch(tol['dist'][s, k], e['dbin'][ai, aj], g['dbin'][ai, aj], RB)
                    _touch(tol['ttc'][s, k], e['tbin'][ai, aj], g['tbin'][ai, aj], TB)
                    if k == 0:
                        nb = {}
                        for name, res in (('e', e), ('g', g)):
                            with np.errstate(invalid='ignore'):
                                md = np.where(res['valid'], res['dist'], np.inf).min(1, initial=np.inf)
                                mt = np.where(res['course'], res['tau'], np.inf).min(1, initial=np.inf)
                            nb[name] = (_min_bin(md, np.float64(np.float32(r_bin)) if name == 'e' else np.float32(r_bin), RB),
                                        _min_bin(mt, np.float64(np.float32(tau_bin)) if name == 'e' else np.float32(tau_bin),
                                                 TB))
                        np.add.at(out['nn'][s], nb['e'][0], 1)
                        np.add.at(out['min_ttc'][s], nb['e'][1], 1)
                        np.add.at(f32['nn'][s], nb['g'][0], 1)
                        np.add.at(f32['min_ttc'][s], nb['g'][1], 1)
                        famb = amb.any(1)
                        fn = famb | (nb['e'][0] != nb['g'][0])
                        fm = famb | (nb['e'][1] != nb['g'][1])
                        _touch(tol['nn'][s], nb['e'][0][fn], nb['g'][0][fn], RB + 1)
                        _touch(tol['min_ttc'][s], nb['e'][1][fm], nb['g'][1][fm], TB + 1)
    out['tol'] = tol
    out['f32'] = f32
    out['n_pairs'] = n_pairs
    out['n_ambiguous'] = n_amb
    return out


def check(got, want, label=''):
    """every output of `got` (dict or object of int arrays) equals want's within want's per-bin tolerance"""
    for k in OUTPUTS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = want[k]
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        bad = np.abs(g - w) > want['tol'][k]
        assert not bad.any(), (label, k, np.argwhere(bad)[:5].tolist(), g[bad][:5].tolist(), w[bad][:5].tolist())
