"""The density-aware floor field restated in numpy float32, beside nav_ref: the deposit of piml_nav_density (deposit), the
slowness of piml_nav_cost (cost) and one weighted Jacobi step of piml_nav_relax_cost (jacobi_step) with its cold-start fixed
point (solve).  Every operation is a single correctly rounded float32 operation, so the kernels' results are these functions'
bit for bit.  two_door_case() is the two-room plan the scheme was first tried on, descend() the walk of its probes."""
import numpy as np

import nav_ref

f32 = np.float32
INF = nav_ref.INF


def deposit(position, mask, x0, y0, cell, gx, gy):
    """position (members, capacity, 2) float32, mask (members, capacity) -> count (members, gy, gx) int32: the present agents
    per cell, an agent's cell being nav_direction's floor((p - origin) / cell) per axis in float32.  Absent slots, NaN
    positions and cells outside the grid deposit nothing."""
    position, mask = np.asarray(position, f32), np.asarray(mask)
    x0, y0, cell = f32(x0), f32(y0), f32(cell)
    count = np.zeros((position.shape[0], gy, gx), np.int32)
    with np.errstate(over='ignore', invalid='ignore'):
        fx = np.floor(((position[..., 0] - x0).astype(f32) / cell).astype(f32))
        fy = np.floor(((position[..., 1] - y0).astype(f32) / cell).astype(f32))
        keep = (mask != 0) & (fx >= 0) & (fx < gx) & (fy >= 0) & (fy < gy)          # (a NaN compares false)
    for m in range(position.shape[0]):
        np.add.at(count[m], (fy[m][keep[m]].astype(np.int64), fx[m][keep[m]].astype(np.int64)), 1)
    return count


def window_sum(count, r):
    """the integer sum of count (..., gy, gx) over the (2r + 1)^2 window of every cell, cells outside the grid counting 0"""
    count = np.asarray(count, np.int64)
    gy, gx = count.shape[-2:]
    pad = np.pad(count, [(0, 0)] * (count.ndim - 2) + [(r, r), (r, r)])
    s = np.zeros_like(count)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            s += pad[..., dy:dy + gy, dx:dx + gx]
    return s


def cost(count, cell, r, kd, rho0, fmax):
    """f (..., gy, gx) float32 = min(1 + kd max(s / area - rho0, 0), fmax), s the window sum, area = (2r + 1)^2 cell^2; also
    rho = s / area.  Blocked cells count in the area."""
    cell, kd, rho0, fmax = f32(cell), f32(kd), f32(rho0), f32(fmax)
    area = f32(f32((2 * r + 1) ** 2) * f32(cell * cell))
    rho = (window_sum(count, r).astype(f32) / area).astype(f32)
    over = np.maximum((rho - rho0).astype(f32), f32(0))
    f = np.minimum((f32(1) + (kd * over).astype(f32)).astype(f32), fmax).astype(f32)
    return f, rho


def jacobi_step(u, blocked, goal, f):
    """nav_ref.jacobi_step with a slowness f (gy, gx) >= 1 per cell: u (G, gy, gx) float32 -> the next iterate"""
    u, f = np.asarray(u, f32), np.asarray(f, f32)[None]
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
        far = ~np.isfinite(hi) | (d >= f)
        root = np.sqrt(((f32(2) * (f * f).astype(f32)).astype(f32) - (d * d).astype(f32)).astype(f32)).astype(f32)
        near = (f32(0.5) * ((lo + hi).astype(f32) + root).astype(f32)).astype(f32)
    cand = np.where(far, (lo + f).astype(f32), near).astype(f32)
    out = np.where(cand < v, cand, v).astype(f32)
    return np.where(fixed0 | fixedi, v, out).astype(f32)


def steps(u, blocked, goal, f, n):
    for _ in range(n):
        u = jacobi_step(u, blocked, goal, f)
    return u


def solve(blocked, goal, f, u=None, max_steps=None):
    """the fixed point from the cold start nav_ref.start(goal) (or from u) and the number of steps that changed something;
    RuntimeError past max_steps (default gx gy + 1)"""
    u = nav_ref.start(goal) if u is None else np.asarray(u, f32)
    limit = goal.shape[1] * goal.shape[2] + 1 if max_steps is None else max_steps
    for n in range(limit + 1):
        nxt = jacobi_step(u, blocked, goal, f)
        if np.array_equal(nxt.view(np.uint32), u.view(np.uint32)):
            return u, n
        u = nxt
    raise RuntimeError('no fixed point')


# ---- the two-room, two-door plan ----
TWO_DOOR_CELL = 0.5
TWO_DOOR_WALL = 20                                          # the wall's column
NEAR_DOOR, FAR_DOOR = (4, 5, 6), (17, 18, 19)               # its open rows
TWO_DOOR_PROBES = ((5, 11), (5, 12), (5, 14), (10, 9), (10, 12), (17, 5), (5, 5))       # (x, y) cells


def two_door_case():
    """40 x 24 (gx x gy), cell 0.5: the border blocked, a wall on column 20 open at rows 4..6 (the near door) and 17..19 (the
    far door), gate 0 the single goal cell (x 36, y 5), and one agent in each cell of rows 3..7, columns 15..19: 25 agents
    queued at the near door.  -> blocked (24, 40) uint8, goal (1, 24, 40) uint8, count (24, 40) int32"""
    gx, gy = 40, 24
    blocked = np.zeros((gy, gx), np.uint8)
    blocked[0], blocked[-1], blocked[:, 0], blocked[:, -1] = 1, 1, 1, 1
    blocked[:, TWO_DOOR_WALL] = 1
    blocked[list(NEAR_DOOR), TWO_DOOR_WALL] = 0
    blocked[list(FAR_DOOR), TWO_DOOR_WALL] = 0
    goal = np.zeros((1, gy, gx), np.uint8)
    goal[0, 5, 36] = 1
    count = np.zeros((gy, gx), np.int32)
    count[3:8, 15:20] = 1
    return blocked, goal, count


def two_door_positions(x0=0.0, y0=0.0, cell=TWO_DOOR_CELL):
    """(25, 2) float32: the centres of the queue's cells"""
    xs, ys = np.meshgrid(np.arange(15, 20), np.arange(3, 8))
    return np.stack([f32(x0) + (xs.ravel().astype(f32) + f32(0.5)) * f32(cell),
                     f32(y0) + (ys.ravel().astype(f32) + f32(0.5)) * f32(cell)], -1).astype(f32)


def descend(u, x, y, column, neighbour=None):
    """Walk from cell (x, y) of plane u (gy, gx) by branch 2's rule of piml_nav_direction (nav_ref.direction's branch 2)
    until the cell lies on `column`; -> its row, or None when no neighbour qualifies first.  neighbour(x, y) -> k replaces
    the rule (the device's answer for the cell's centre)."""
    gy, gx = u.shape
    for _ in range(gx * gy):
        if x == column:
            return y
        k = _descent(u, x, y) if neighbour is None else neighbour(x, y)
        if k < 0:
            return None
        x, y = x + nav_ref.NEIGHBOURS[k][0], y + nav_ref.NEIGHBOURS[k][1]
    return None


def _descent(u, cx, cy):
    """branch 2's neighbour of cell (cx, cy): nav_ref.direction's loop, -1 when none qualifies"""
    u3 = u[None]
    uc = u[cy, cx]
    if not np.isfinite(uc):
        return -1
    best, k = f32(0), -1
    fin = lambda dx, dy: bool(np.isfinite(nav_ref._u(u3, 0, cx + dx, cy + dy)))
    for j, (dx, dy) in enumerate(nav_ref.NEIGHBOURS):
        un = nav_ref._u(u3, 0, cx + dx, cy + dy)
        if not np.isfinite(un) or (dx and dy and not (fin(dx, 0) and fin(0, dy))):
            continue
        s = f32(uc - un) if not (dx and dy) else f32(f32(uc - un) * nav_ref.DIAG)
        if s > best:
            best, k = s, j
    return k
