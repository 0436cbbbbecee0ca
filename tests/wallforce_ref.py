"""numpy restatement of the wall term (include/piml_hip.h, piml_wall_force): the selection by brute force over ALL valid
obstacle points in float32, operation by operation -- d2 = fadd(fmul(e.x, e.x), fmul(e.y, e.y)), the minimum of the key
(bits(d2) << 32) | sorted index, the predicate d2 < c2 = fl(cutoff cutoff) -- and the force value in float64 on the
float32-selected point.  It knows nothing of cells except the order they put the points in (the tie rule), which
`sorted_points` restates on its own."""
import numpy as np

f32 = np.float32
MARGIN = f32(1.0 + 2.0 ** -5)


def sorted_points(obstacles, cutoff, cell=None):
    """(points, order): the valid points in the grid's order -- by cell index cy gx + cx, stably -- and their indices into
    `obstacles`.  cell: the grid's cell side when it was coarsened (default cutoff (1 + 2^-5) in float32)."""
    obs = np.asarray(obstacles, f32).reshape(-1, 2)
    keep = np.flatnonzero(np.isfinite(obs).all(1))
    pts = obs[keep]
    if pts.shape[0] == 0:
        return pts, keep
    cell = f32(f32(cutoff) * MARGIN) if cell is None else f32(cell)
    c = np.floor((pts - pts.min(0)) / cell).astype(np.int64)
    gx = int(c[:, 0].max()) + 1
    order = np.argsort(c[:, 1] * gx + c[:, 0], kind='stable')
    return pts[order], keep[order]


def select(position, points, cutoff, chunk=1024):
    """(index (n) int32, dist2 (n) float32) of every row of position (n, 2) float32 against `points` (in sorted order):
    the nearest point under the float32 d2, ties to the lower index, kept when d2 < c2; otherwise (-1, +inf) -- also for a
    NaN position."""
    P = np.asarray(position, f32).reshape(-1, 2)
    Q = np.asarray(points, f32).reshape(-1, 2)
    n = P.shape[0]
    index = np.full(n, -1, np.int32)
    dist2 = np.full(n, np.inf, f32)
    if Q.shape[0] == 0:
        return index, dist2
    c2 = f32(cutoff) * f32(cutoff)
    ids = np.arange(Q.shape[0], dtype=np.uint64)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, n, chunk):
            p = P[a:a + chunk]
            ex = Q[None, :, 0] - p[:, None, 0]
            ey = Q[None, :, 1] - p[:, None, 1]
            d2 = ex * ex + ey * ey                               # float32: two products, one add, each rounded
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]
            key[np.isnan(d2)] = np.uint64(0xFFFFFFFFFFFFFFFF)
            k = key.min(1)
            best = (k >> np.uint64(32)).astype(np.uint32).view(f32)
            felt = (k != np.uint64(0xFFFFFFFFFFFFFFFF)) & (best < c2) & ~np.isnan(p).any(1)
            index[a:a + chunk] = np.where(felt, (k & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
            dist2[a:a + chunk] = np.where(felt, best, f32(np.inf))
    return index, dist2


def force(position, points, index, A, B):
    """W = A exp(B d) (p - q) / d in float64 for the selected points (zero for index -1 and for d == 0): (n, 2) float64."""
    P = np.asarray(position, np.float64).reshape(-1, 2)
    Q = np.asarray(points, np.float64).reshape(-1, 2)
    out = np.zeros_like(P)
    ok = np.flatnonzero(index >= 0)
    e = P[ok] - Q[index[ok]]
    d = np.sqrt((e * e).sum(1))
    pos = d > 0
    w = np.zeros_like(e)
    w[pos] = (float(A) * np.exp(float(B) * d[pos]) / d[pos])[:, None] * e[pos]
    out[ok] = w
    return out


def check_force(got, want, A, label=''):
    """the bar of the smooth law (mlapm.hpp): 1e-5 relative of the float64 value, with an absolute floor of 1e-6 A"""
    got, want = np.asarray(got, np.float64).reshape(-1, 2), np.asarray(want, np.float64).reshape(-1, 2)
    tol = 1e-5 * np.sqrt((want * want).sum(1)) + 1e-6 * float(A)
    err = np.abs(got - want).max(1)
    worst = int(np.argmax(err - tol)) if err.size else 0
    assert (err <= tol).all(), (label, worst, got[worst], want[worst])
    return float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
