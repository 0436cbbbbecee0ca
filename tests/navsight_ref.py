"""The any-angle floor field restated in numpy float32 and Python integers: visible(c, q), the integer sight test of
piml_nav_sight_relax; one Jacobi step of its Theta*-style propagation (jacobi_step) -- w is one correctly rounded float32
add of a correctly rounded float32 root, parent an index, so the kernel's planes are this function's bit for bit --; its
fixed point (solve); and the lookup's branch 3 (direction) on top of nav_ref.direction.  As in nav_ref a goal cell is free
whatever `blocked` says: every gate sees the mask blocked & ~goal[g]."""
import numpy as np

import nav_ref

f32 = np.float32
INF = f32(np.inf)
NEIGHBOURS = nav_ref.NEIGHBOURS


def _axis(a, D):
    """the two strict bounds l < t < u that |a - t D| < 1 - t / 2 puts on t, as fractions (ln, ld, un, ud) with ld, ud > 0:
    t (2 D - 1) > 2 a - 2 and t (2 D + 1) < 2 a + 2.  D < 0 mirrors the axis; D == 0 leaves t < 2 - 2 |a| and no lower bound
    (-1 stands for it: t >= 0 anyway)"""
    if D < 0:
        a, D = -a, -D
    if D == 0:
        return -1, 1, 2 - 2 * abs(a), 1
    return 2 * a - 2, 2 * D - 1, 2 * a + 2, 2 * D + 1


def obstructs(ax, ay, Dx, Dy):
    """True when the open unit square at offset a from c meets the hull of c's square and the point at offset D: a t in
    [0, 1] between every lower and every upper bound of both axes, by integer cross-multiplication"""
    lxn, lxd, uxn, uxd = _axis(ax, Dx)
    lyn, lyd, uyn, uyd = _axis(ay, Dy)
    return (lxn * uxd < uxn * lxd and lxn * uyd < uyn * lxd and lyn * uxd < uxn * lyd and lyn * uyd < uyn * lyd
            and lxn < lxd and lyn < lyd and uxn > 0 and uyn > 0)


def visible(mask, c, q, pad=None):
    """mask (gy, gx) nonzero = blocked, outside the grid blocked; c, q = (x, y) inside the grid.  Only the cells of the
    bounding box of c and q grown by one cell can obstruct.  pad: the mask padded by one blocked cell, to save the copy"""
    (cx, cy), (qx, qy) = c, q
    Dx, Dy = qx - cx, qy - cy
    if pad is None:
        pad = np.pad(np.asarray(mask) != 0, 1, constant_values=True)     # pad[y + 1, x + 1] = cell (x, y)
    x_lo, y_lo = min(cx, qx) - 1, min(cy, qy) - 1
    ys, xs = np.nonzero(pad[y_lo + 1:max(cy, qy) + 3, x_lo + 1:max(cx, qx) + 3])
    return not any(obstructs(int(x) + x_lo - cx, int(y) + y_lo - cy, Dx, Dy) for x, y in zip(xs, ys))


class Sight:
    """visible() of one static mask, remembered per pair (it is a property of the mask alone)"""

    def __init__(self, mask):
        self.mask, self.memo = np.asarray(mask) != 0, {}
        self.pad = np.pad(self.mask, 1, constant_values=True)

    def __call__(self, c, q):
        k = (c, q)
        if k not in self.memo:
            self.memo[k] = visible(self.mask, c, q, self.pad)
        return self.memo[k]


def dist(c, q):
    """sqrtf((float)(dx dx + dy dy)): the integer is exact in float32, the root correctly rounded"""
    dx, dy = q[0] - c[0], q[1] - c[1]
    return f32(np.sqrt(f32(dx * dx + dy * dy)))


def start(goal):
    """w: 0 on goal cells, +inf elsewhere; parent: self on goal cells, -1 elsewhere"""
    G, gy, gx = goal.shape
    w = np.where(goal != 0, f32(0), INF).astype(f32)
    lin = np.arange(gy * gx, dtype=np.int32).reshape(gy, gx)
    parent = np.where(goal != 0, lin[None], np.int32(-1)).astype(np.int32)
    return w, parent


def sights(blocked, goal):
    """one Sight per gate, over blocked & ~goal[g]"""
    return [Sight((np.asarray(blocked) != 0) & ~(goal[g] != 0)) for g in range(goal.shape[0])]


def jacobi_step(w, parent, blocked, goal, sight=None):
    """(w, parent) (G, gy, gx) -> the next Jacobi iterate.  sight: sights(blocked, goal) to share the memo across steps"""
    G, gy, gx = goal.shape
    sight = sights(blocked, goal) if sight is None else sight
    w2, p2 = w.copy(), parent.copy()
    for g in range(G):
        mask, vis, wg, pg = sight[g].mask, sight[g], w[g], parent[g]
        free = lambda x, y: 0 <= x < gx and 0 <= y < gy and not mask[y, x]
        fin = np.isfinite(wg)
        pad = np.pad(fin, 1)                                # a cell without a finite cell in its 3 x 3 block has no parent
        near = np.zeros_like(fin)                           # and no candidate: it stays (+inf, -1)
        for dy in range(3):
            for dx in range(3):
                near |= pad[dy:dy + gy, dx:dx + gx]
        for y, x in zip(*np.nonzero(near & ~mask & (goal[g] == 0))):
            x, y = int(x), int(y)
            c = (x, y)
            best, bp = INF, -1
            q = int(pg[y, x])
            if q >= 0:
                qc = (q % gx, q // gx)
                best, bp = f32(wg[qc[1], qc[0]] + dist(c, qc)), q
            for dx, dy in NEIGHBOURS:
                nx, ny = x + dx, y + dy
                if not free(nx, ny) or not fin[ny, nx]:
                    continue
                if dx and dy and not (free(x + dx, y) and free(x, y + dy)):
                    continue
                q = int(pg[ny, nx])
                qc = (q % gx, q // gx)
                if not vis(c, qc):
                    q, qc = ny * gx + nx, (nx, ny)
                cand = f32(wg[qc[1], qc[0]] + dist(c, qc))
                if cand < best:
                    best, bp = cand, q
            w2[g, y, x], p2[g, y, x] = best, bp
    return w2, p2


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def steps(blocked, goal, n, sight=None):
    """the state after n steps from start(goal)"""
    sight = sights(blocked, goal) if sight is None else sight
    s = start(goal)
    for _ in range(n):
        s = jacobi_step(*s, blocked, goal, sight)
    return s


def solve(blocked, goal, sight=None):
    """the fixed point from start(goal): (w, parent, the number of steps that changed something)"""
    sight = sights(blocked, goal) if sight is None else sight
    s = start(goal)
    for n in range(goal.shape[1] * goal.shape[2] + 2):
        nxt = jacobi_step(*s, blocked, goal, sight)
        if same(nxt, s):
            return s[0], s[1], n
        s = nxt
    raise RuntimeError('no fixed point')


def chain(parent_g, c):
    """the cells (x, y) from c's parent to the gate cell that is its own parent"""
    gx = parent_g.shape[1]
    out, lin = [], c[1] * gx + c[0]
    while True:
        q = int(parent_g[lin // gx, lin % gx])
        if q < 0 or q == lin:
            return out
        out.append((q % gx, q // gx))
        lin = q


def direction(u, parent, x0, y0, cell, near, P, gate, dest, base=None):
    """nav_ref.direction with branch 3 in front of branches 1 and 2: where the first-order field applies (p inside the grid,
    the gate valid, u[c] finite and > near) and parent[g][c] = q >= 0 is not c, e points from p to q's centre, the branch is 3
    and the neighbour -1.  e float64, branch and neighbour exact.  base: nav_ref.direction's result for the same rows, if the
    caller has it"""
    e, branch, nb = (np.array(a) for a in (nav_ref.direction(u, x0, y0, cell, near, P, gate, dest) if base is None else base))
    u = np.asarray(u, f32)
    G, gy, gx = u.shape
    x0, y0, cell, near = f32(x0), f32(y0), f32(cell), f32(near)
    P = np.asarray(P, f32)
    for r in range(P.shape[0]):
        p, g = P[r], int(gate[r])
        if np.isnan(p).any() or not 0 <= g < G:
            continue
        with np.errstate(over='ignore', invalid='ignore'):
            fcx, fcy = np.floor(f32(f32(p[0] - x0) / cell)), np.floor(f32(f32(p[1] - y0) / cell))
        if not (0 <= fcx < gx and 0 <= fcy < gy):
            continue
        cx, cy = int(fcx), int(fcy)
        uc = u[g, cy, cx]
        if not np.isfinite(uc) or uc <= near:
            continue
        q = int(parent[g, cy, cx])
        if q < 0 or q == cy * gx + cx:
            continue
        hx = f32(f32(x0 + f32(f32(f32(q % gx) + f32(0.5)) * cell)) - p[0])
        hy = f32(f32(y0 + f32(f32(f32(q // gx) + f32(0.5)) * cell)) - p[1])
        if not f32(f32(hx * hx) + f32(hy * hy)) > 0:
            continue
        v = np.array([hx, hy], np.float64)
        e[r], branch[r], nb[r] = v / np.hypot(*v), 3, -1
    return e, branch, nb


def u_wall_case():
    """33 x 33, goal (16, 16) inside a U-shaped wall open to the left: blocked x = 20 for y in 8..24, and y = 8 and y = 24
    for x in 10..20"""
    blocked = np.zeros((33, 33), np.uint8)
    blocked[8:25, 20] = 1
    blocked[8, 10:21] = 1
    blocked[24, 10:21] = 1
    goal = np.zeros((1, 33, 33), np.uint8)
    goal[0, 16, 16] = 1
    return blocked, goal
