"""The floor field restated in numpy float32: one Jacobi step of piml_nav_relax (jacobi_step) -- every operation a single
correctly rounded float32 operation, so the kernel's result is this function's bit for bit -- its fixed point (solve), and the
three-branch lookup of piml_nav_direction (direction), whose branch and neighbour are exact and whose value is float64."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
DIAG = f32(0.70710678118654752)
# branch 2's neighbours in the header's order: E, W, N, S, NE, NW, SE, SW (N = +y)
NEIGHBOURS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))


def start(goal):
    """0 on goal cells, +inf elsewhere: (G, gy, gx) float32"""
    return np.where(goal != 0, f32(0), INF).astype(f32)


def jacobi_step(u, blocked, goal):
    """u (G, gy, gx) float32 -> the next Jacobi iterate; goal cells 0, other blocked cells +inf, outside the grid +inf"""
    u = np.asarray(u, f32)
    fixed0 = goal != 0
    fixedi = (blocked != 0)[None] & ~fixed0
    v = np.where(fixed0, f32(0), np.where(fixedi, INF, u)).astype(f32)
    pad = np.pad(v, ((0, 0), (1, 1), (1, 1)), constant_values=INF)
    left, right = pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]
    down, up = pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]
    a = np.where(left < right, left, right)
    b = np.where(down < up, down, up)
    lo = np.where(a < b, a, b)
    hi = np.where(a < b, b, a)
    with np.errstate(invalid='ignore'):
        d = (hi - lo).astype(f32)
        far = ~np.isfinite(hi) | (d >= f32(1))
        near = (f32(0.5) * ((lo + hi).astype(f32) + np.sqrt((f32(2) - (d * d).astype(f32)).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    cand = np.where(far, (lo + f32(1)).astype(f32), near).astype(f32)
    out = np.where(cand < v, cand, v).astype(f32)
    return np.where(fixed0 | fixedi, v, out).astype(f32)


def steps(u, blocked, goal, n):
    for _ in range(n):
        u = jacobi_step(u, blocked, goal)
    return u


def solve(blocked, goal, max_steps=None):
    """the fixed point from start(goal) and the number of steps that changed something"""
    u = start(goal)
    limit = goal.shape[1] * goal.shape[2] + 1 if max_steps is None else max_steps
    for n in range(limit + 1):
        nxt = jacobi_step(u, blocked, goal)
        if np.array_equal(nxt.view(np.uint32), u.view(np.uint32)):
            return u, n
        u = nxt
    raise RuntimeError('no fixed point')


def _u(u, g, x, y):
    gy, gx = u.shape[1:]
    return u[g, y, x] if 0 <= x < gx and 0 <= y < gy else INF


def direction(u, x0, y0, cell, near, P, gate, dest, skip_rule=True):
    """e (n, 2) float64, branch (n) int32, neighbour (n) int32 of piml_nav_direction for rows P (n, 2), gate (n), dest (n, 2).
    skip_rule=False drops branch 2's rule that a diagonal is skipped beside a cell that is not finite (to show where it binds)"""
    u = np.asarray(u, f32)
    G, gy, gx = u.shape
    x0, y0, cell, near = f32(x0), f32(y0), f32(cell), f32(near)
    P, dest = np.asarray(P, f32), np.asarray(dest, f32)
    n = P.shape[0]
    e, branch, nb = np.zeros((n, 2)), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for r in range(n):
        p, g = P[r], int(gate[r])
        with np.errstate(invalid='ignore'):
            s = dest[r].astype(np.float64) - p.astype(np.float64)
            e[r] = s / max(np.hypot(*s), 1e-12)
        if np.isnan(p).any() or not 0 <= g < G:
            continue
        with np.errstate(over='ignore', invalid='ignore'):
            qx, qy = f32(f32(p[0] - x0) / cell), f32(f32(p[1] - y0) / cell)
        fcx, fcy = np.floor(qx), np.floor(qy)
        if not (0 <= fcx < gx and 0 <= fcy < gy):
            continue
        cx, cy = int(fcx), int(fcy)
        uc = u[g, cy, cx]
        if not np.isfinite(uc) or uc <= near:
            continue
        fx, fy = f32(qx - f32(0.5)), f32(qy - f32(0.5))
        fi, fj = np.floor(fx), np.floor(fy)
        if 0 <= fi <= gx - 2 and 0 <= fj <= gy - 2:
            i0, j0 = int(fi), int(fj)
            u00, u10, u01, u11 = u[g, j0, i0], u[g, j0, i0 + 1], u[g, j0 + 1, i0], u[g, j0 + 1, i0 + 1]
            if np.isfinite([u00, u10, u01, u11]).all():
                tx, ty = f32(fx - fi), f32(fy - fj)
                gxv = f32(f32(f32(f32(1) - ty) * f32(u10 - u00)) + f32(ty * f32(u11 - u01)))
                gyv = f32(f32(f32(f32(1) - tx) * f32(u01 - u00)) + f32(tx * f32(u11 - u10)))
                n2 = f32(f32(gxv * gxv) + f32(gyv * gyv))
                if n2 > 0:
                    v = -np.array([gxv, gyv], np.float64)
                    e[r], branch[r] = v / np.hypot(*v), 1
                    continue
        best, k = f32(0), -1
        fin = lambda dx, dy: bool(np.isfinite(_u(u, g, cx + dx, cy + dy)))
        for j, (dx, dy) in enumerate(NEIGHBOURS):
            un = _u(u, g, cx + dx, cy + dy)
            if not np.isfinite(un) or (skip_rule and dx and dy and not (fin(dx, 0) and fin(0, dy))):
                continue
            s_ = f32(uc - un) if not (dx and dy) else f32(f32(uc - un) * DIAG)
            if s_ > best:
                best, k = s_, j
        if k < 0:
            continue
        dx, dy = NEIGHBOURS[k]
        hx = f32(f32(x0 + f32(f32(f32(cx + dx) + f32(0.5)) * cell)) - p[0])
        hy = f32(f32(y0 + f32(f32(f32(cy + dy) + f32(0.5)) * cell)) - p[1])
        if not f32(f32(hx * hx) + f32(hy * hy)) > 0:
            continue
        v = np.array([hx, hy], np.float64)
        e[r], branch[r], nb[r] = v / np.hypot(*v), 2, k
    return e, branch, nb


def u_shape_case():
    """33 x 34 (gx x gy): a U-shaped wall open to the top, gate 0 inside the U, gate 1 outside at the bottom left with one of
    its two goal cells on a blocked cell, and one free cell walled in on all four sides.  -> blocked (34, 33), goal (2, 34, 33)"""
    gx, gy = 33, 34
    blocked = np.zeros((gy, gx), np.uint8)
    blocked[5:30, 8] = 1
    blocked[5:30, 26] = 1
    blocked[5, 8:27] = 1
    blocked[19, 30], blocked[21, 30], blocked[20, 29], blocked[20, 31] = 1, 1, 1, 1      # (x 30, y 20) is enclosed
    goal = np.zeros((2, gy, gx), np.uint8)
    goal[0, 8, 17] = 1
    goal[1, 1, 1] = 1
    goal[1, 5, 8] = 1                                            # a goal on a blocked cell: free for gate 1
    return blocked, goal
