"""A numpy restatement of the Voronoi cell of piml_crowd_stats_voronoi (include/piml_hip.h), float64 by
default: the same start polygon from the same directions, the same clip order and skip rules, the same intersection
formula, and no capacity limit.  `dtype=np.float32` runs the same code in float32 (every operation rounded as the device
rounds it; the shoelace sum stays float64, as on the device)."""
import numpy as np


def clip(poly, s, axis=-1, snap=0.0):
    """One Sutherland-Hodgman round: poly (n, 2), s (n) signed distances; keeps s <= 0.  Edge l -> l + 1 emits vertex l when
    it is inside and, when its ends differ, v_in + t (v_out - v_in) with t = s_in / (s_in - s_out); axis 0 / 1: that
    point's x / y is `snap` itself."""
    inside = s <= 0
    if inside.all():
        return poly
    nxt = np.roll(np.arange(len(poly)), -1)
    cross = inside != inside[nxt]
    a = np.where(inside, np.arange(len(poly)), nxt)[cross]          # the inside end
    b = np.where(inside, nxt, np.arange(len(poly)))[cross]
    t = s[a] / (s[a] - s[b])
    pts = poly[a] + t[:, None] * (poly[b] - poly[a])
    if axis >= 0:
        pts[:, axis] = snap
    count = inside.astype(np.int64) + cross
    at = np.cumsum(count) - count
    out = np.empty((int(count.sum()), 2), poly.dtype)
    out[at[inside]] = poly[inside]
    out[(at + inside)[cross]] = pts
    return out


def shoelace(poly):
    """float64 area of (n, 2) vertices of any float type (exact products, as the device forms them)."""
    if len(poly) == 0:
        return 0.0
    p = poly.astype(np.float64)
    q = np.roll(p, -1, 0)
    return 0.5 * float(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]))


def focal_mask(P, M, box=None, bounds=None, n_active=None):
    """(present, focal) of one slice: P (N, 2), M (N)."""
    P = np.asarray(P, np.float32)
    present = (np.asarray(M) == 1) & np.isfinite(P).all(1)
    if n_active is not None:
        present &= np.arange(len(P)) < n_active
    focal = present.copy()
    with np.errstate(invalid='ignore'):
        for rect in (box, bounds):
            if rect is not None:
                x0, x1, y0, y1 = (np.float32(v) for v in rect)
                focal &= (P[:, 0] >= x0) & (P[:, 0] < x1) & (P[:, 1] >= y0) & (P[:, 1] < y1)
    return present, focal


def cells(P, M, cutoff, dirs, bounds=None, box=None, n_active=None, dtype=np.float64):
    """The cells of one slice.  Returns (area (N) float64, NaN where the agent is not focal; vertices (N) of the final
    polygon; peak (N) the largest vertex count after any clip), arithmetic in `dtype`."""
    P32 = np.asarray(P, np.float32)
    present, focal = focal_mask(P32, M, box, bounds, n_active)
    N = len(P32)
    area, verts, peak = np.full(N, np.nan), np.zeros(N, np.int64), np.zeros(N, np.int64)
    src = P32[present].astype(dtype)                               # slot order
    c = dtype(np.float32(cutoff))
    start = c * np.asarray(dirs, np.float32).astype(dtype)
    four_c2 = dtype(4) * (c * c)
    rect = None if bounds is None else [dtype(np.float32(v)) for v in bounds]
    for i in np.flatnonzero(focal):
        p = P32[i].astype(dtype)
        poly = start.copy()
        top = len(poly)
        if rect is not None:
            hx0, hx1, hy0, hy1 = rect[0] - p[0], rect[1] - p[0], rect[2] - p[1], rect[3] - p[1]
            for s_of, axis, snap in ((lambda g: hx0 - g[:, 0], 0, hx0), (lambda g: g[:, 0] - hx1, 0, hx1),
                                     (lambda g: hy0 - g[:, 1], 1, hy0), (lambda g: g[:, 1] - hy1, 1, hy1)):
                if len(poly):
                    poly = clip(poly, s_of(poly), axis, snap)
                    top = max(top, len(poly))
        d = src - p
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        cand = np.flatnonzero((d2 != 0) & (d2 < four_c2))
        while len(cand) and len(poly):
            # the signed distances of the current polygon to every bisector still to come: those before the first one
            # that cuts leave the polygon as it is, so the clips are applied one by one in slot order all the same
            s = (poly[:, 0, None] * d[cand, 0] + poly[:, 1, None] * d[cand, 1]) - dtype(0.5) * d2[cand]
            cuts = ~(s <= 0).all(0)
            if not cuts.any():
                break
            k = int(np.argmax(cuts))
            poly = clip(poly, s[:, k])
            top = max(top, len(poly))
            cand = cand[k + 1:]
        area[i], verts[i], peak[i] = shoelace(poly), len(poly), top
    return area, verts, peak


def rho_of(area):
    """The float32 density of float64 areas as the device forms it: the area rounded to float32, rho = 1 / area a float32
    division; NaN where the rounded area is not > 0."""
    a32 = np.asarray(area, np.float64).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(a32 > 0, np.float32(1) / a32, np.float32(np.nan)).astype(np.float32)


def cells_frames(P, M, cutoff, dirs, bounds=None, box=None, n_active=None, dtype=np.float64):
    """cells over (T, N, .) frames: (area, vertices, peak), each (T, N)."""
    out = [cells(P[t], M[t], cutoff, dirs, bounds, box, n_active, dtype) for t in range(len(P))]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))
