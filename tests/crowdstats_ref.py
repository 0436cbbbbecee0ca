"""Float64 numpy restatement of the crowd statistics (piml_amd.crowdstats).  The density is float64 over
the float32 positions; the bins and cells are computed in float32 exactly as specified.  `rho` may be given (the device's
float32 densities, (S, T', N)) so that everything downstream of it can be checked exactly."""
import math

import numpy as np


def grid_shape(box, cell):
    x0, x1, y0, y1 = (float(np.float32(v)) for v in box)
    h = float(np.float32(cell))
    return int(math.ceil((x1 - x0) / h)), int(math.ceil((y1 - y0) / h))


def crowd_stats(P, V, M, radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=24, frames=None, n_active=None, rho=None):
    P, V, M = (np.asarray(x, np.float32) for x in (P, V, M))
    if P.ndim == 3:
        P, V, M = P[None], V[None], M[None]
    S, T, N = M.shape
    a, b = frames if frames is not None else (0, T)
    Tp, B = b - a, rho_bins
    R = np.float64(np.float32(radius))
    gx, gy = grid_shape(box, cell) if box is not None else (0, 0)
    bx = None if box is None else [np.float32(v) for v in box]
    h = np.float32(cell)
    out = dict(n=np.zeros((S, Tp), np.int64), n_speed=np.zeros((S, Tp), np.int64), sum_speed=np.zeros((S, Tp)),
               sum_density=np.zeros((S, Tp)), fd_count=np.zeros((S, B), np.int64), fd_sum=np.zeros((S, B)),
               fd_sum2=np.zeros((S, B)), map=np.zeros((S, gy, gx), np.int64) if box is not None else None,
               density=np.full((S, Tp, N), np.nan, np.float32))
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        for k in range(Tp):
            p, v, m = P[s, a + k, :bound], V[s, a + k, :bound], M[s, a + k, :bound]
            present = (m == 1) & np.isfinite(p).all(1)
            focal = present.copy()
            if bx is not None:
                focal &= (bx[0] <= p[:, 0]) & (p[:, 0] < bx[1]) & (bx[2] <= p[:, 1]) & (p[:, 1] < bx[3])
            idx = np.nonzero(focal)[0]
            if rho is None:
                q = p[present].astype(np.float64)
                r = np.empty(len(idx), np.float32)
                for c in range(0, len(idx), 256):                   # focal rows in chunks (memory)
                    pi = p[idx[c:c + 256]].astype(np.float64)
                    d2 = ((pi[:, None, :] - q[None, :, :]) ** 2).sum(-1)
                    r[c:c + 256] = np.exp(-d2 / (R * R)).sum(1) / (np.pi * R * R)
            else:
                r = np.asarray(rho, np.float32)[s, k, idx]
            out['density'][s, k, idx] = r
            out['n'][s, k] = len(idx)
            out['sum_density'][s, k] = r.astype(np.float64).sum()
            vi = v[idx]
            sp = np.isfinite(vi).all(1)
            u = np.sqrt(vi[sp, 0] * vi[sp, 0] + vi[sp, 1] * vi[sp, 1])          # float32
            out['n_speed'][s, k] = sp.sum()
            out['sum_speed'][s, k] = u.astype(np.float64).sum()
            binf = np.floor(r[sp] / np.float32(rho_bin))
            bins = np.where(binf >= np.float32(B - 1), B - 1, binf).astype(np.int64)
            np.add.at(out['fd_count'][s], bins, 1)
            np.add.at(out['fd_sum'][s], bins, u.astype(np.float64))
            np.add.at(out['fd_sum2'][s], bins, u.astype(np.float64) ** 2)
            if box is not None:
                pf = p[idx]
                cx = np.floor((pf[:, 0] - bx[0]) / h)
                cy = np.floor((pf[:, 1] - bx[2]) / h)
                ok = (cx >= 0) & (cx < gx) & (cy >= 0) & (cy < gy)
                np.add.at(out['map'][s], (cy[ok].astype(np.int64), cx[ok].astype(np.int64)), 1)
    return out
