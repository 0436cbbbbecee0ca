"""The direction-aware density of the floor field restated in numpy float32, beside nav_ref and navcost_ref: the descent
direction of piml_nav_descent (descent_dir), the deposit of piml_nav_flow (deposit_flow) and the slowness per gate of
piml_nav_cost_flow (cost_flow).  Every operation is a single correctly rounded float32 operation and every sum an integer, so
the kernels' results are these functions' bit for bit.  The solve per gate is navcost_ref.solve with that gate's plane
(solve_gates)."""
import numpy as np

import nav_ref
import navcost_ref

f32 = np.float32
INF = nav_ref.INF
Q_UNIT = f32(1024)                                          # the momentum planes count 2^-10 m/s
V_CLAMP = f32(8)
GATE1_PROBES = ((35, 11), (35, 12), (35, 14), (30, 9), (30, 12), (23, 5), (35, 5))      # (x, y) cells, bound for gate 1


def descent_dir(u):
    """u (G, gy, gx) float32, the STATIC field -> d (G, gy, gx, 2) float32: the upwind unit direction of steepest descent;
    (0, 0) on goal cells, where u = +inf (blocked and unreachable cells) and on plateaus"""
    u = np.asarray(u, f32)
    pad = np.pad(u, ((0, 0), (1, 1), (1, 1)), constant_values=INF)
    L, R = pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]
    D, U = pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]
    a = np.where(L < R, L, R)
    b = np.where(D < U, D, U)
    with np.errstate(invalid='ignore', divide='ignore'):
        rx = np.where(np.isfinite(u) & np.isfinite(a) & (a < u), (u - a).astype(f32), f32(0)).astype(f32)
        ry = np.where(np.isfinite(u) & np.isfinite(b) & (b < u), (u - b).astype(f32), f32(0)).astype(f32)
        rx = np.where(L < R, -rx, rx).astype(f32)
        ry = np.where(D < U, -ry, ry).astype(f32)
        n = np.sqrt(((rx * rx).astype(f32) + (ry * ry).astype(f32)).astype(f32)).astype(f32)
        dx = np.where(n > 0, (rx / n).astype(f32), f32(0))
        dy = np.where(n > 0, (ry / n).astype(f32), f32(0))
    return np.stack([dx, dy], -1).astype(f32)


def quantise(v):
    """a velocity component in 2^-10 m/s: 0 when not finite, else clamped to +-8 m/s and rounded half to even"""
    v = np.asarray(v, f32)
    with np.errstate(invalid='ignore'):
        q = np.rint((np.minimum(np.maximum(v, -V_CLAMP), V_CLAMP).astype(f32) * Q_UNIT).astype(f32))
    return np.where(np.isfinite(v), q, 0).astype(np.int32)


def deposit_flow(position, velocity, mask, x0, y0, cell, gx, gy):
    """position, velocity (members, capacity, 2) float32, mask (members, capacity) -> count (members, gy, gx) int32 --
    navcost_ref.deposit's -- and mom (members, 2, gy, gx) int32, the quantised velocity components of the slots that count"""
    position, velocity, mask = np.asarray(position, f32), np.asarray(velocity, f32), np.asarray(mask)
    x0, y0, cell = f32(x0), f32(y0), f32(cell)
    M = position.shape[0]
    count = np.zeros((M, gy, gx), np.int32)
    mom = np.zeros((M, 2, gy, gx), np.int32)
    with np.errstate(over='ignore', invalid='ignore'):
        fx = np.floor(((position[..., 0] - x0).astype(f32) / cell).astype(f32))
        fy = np.floor(((position[..., 1] - y0).astype(f32) / cell).astype(f32))
        keep = (mask != 0) & (fx >= 0) & (fx < gx) & (fy >= 0) & (fy < gy)
    q = quantise(velocity)
    for m in range(M):
        iy, ix = fy[m][keep[m]].astype(np.int64), fx[m][keep[m]].astype(np.int64)
        np.add.at(count[m], (iy, ix), 1)
        np.add.at(mom[m, 0], (iy, ix), q[m, :, 0][keep[m]])
        np.add.at(mom[m, 1], (iy, ix), q[m, :, 1][keep[m]])
    assert np.array_equal(count, navcost_ref.deposit(position, mask, x0, y0, cell, gx, gy))
    return count, mom


def cost_flow(count, mom, d, cell, r, kd, rho0, fmax, flow, vref):
    """count (members, gy, gx), mom (members, 2, gy, gx) int32, d (G, gy, gx, 2) float32 -> f (members, G, gy, gx) float32:
    navcost_ref.cost with the head count s replaced by s_eff = s - flow (p . d) / (1024 vref), p the window sums of mom"""
    cell, kd, rho0, fmax, flow, vref = f32(cell), f32(kd), f32(rho0), f32(fmax), f32(flow), f32(vref)
    d = np.asarray(d, f32)
    area = f32(f32((2 * r + 1) ** 2) * f32(cell * cell))
    s = navcost_ref.window_sum(count, r).astype(f32)[:, None]                   # (members, 1, gy, gx)
    p = navcost_ref.window_sum(mom, r).astype(f32)                              # (members, 2, gy, gx)
    px, py = p[:, None, 0], p[:, None, 1]
    dx, dy = d[None, ..., 0], d[None, ..., 1]
    with np.errstate(over='ignore', invalid='ignore'):
        pd = ((px * dx).astype(f32) + (py * dy).astype(f32)).astype(f32)
        along = (pd / f32(Q_UNIT * vref)).astype(f32)
        s_eff = (s - (flow * along).astype(f32)).astype(f32)
        over = np.maximum(((s_eff / area).astype(f32) - rho0).astype(f32), f32(0))
        return np.minimum((f32(1) + (kd * over).astype(f32)).astype(f32), fmax).astype(f32)


def solve_gates(blocked, goal, f):
    """f (G, gy, gx): one member's cost plane per gate -> (u (G, gy, gx), the steps per gate): navcost_ref.solve per gate"""
    out = [navcost_ref.solve(blocked, goal[g:g + 1], f[g]) for g in range(goal.shape[0])]
    return np.concatenate([u for u, _ in out]), [n for _, n in out]


def two_door_two_gates():
    """navcost_ref.two_door_case() with a second gate whose single goal cell is (x 3, y 5), in the queue's room: gate 0 lies
    through the wall in the direction +x of the queue, gate 1 behind it.  -> blocked, goal (2, 24, 40), count"""
    blocked, goal, count = navcost_ref.two_door_case()
    goal = np.concatenate([goal, np.zeros_like(goal)])
    goal[1, 5, 3] = 1
    return blocked, goal, count
