"""numpy float32 restatement of the exit choice (piml_nav_choose_exit, piml_amd/csrc/scenario.hip) for the tests: the rule as a
function from (state, field, classes, law, t) to the new state.

state: a dict of numpy arrays of ONE member -- p, dest (cap, 2) float32, flag (cap) int32, mask (cap) float32, waypoints
(D, cap, 2) float32, exit_idx (D, cap) int32 -- and n, the agents spawned through frame t (spawned[t & 1]).  u (G, gy, gx)
float32 in cell units is that member's field.  margin and commit are in CELL units (cells()).

Per slot i < min(n, cap) with mask != 0 and f = flag[i] in 0..1, cur = exit_idx[f][i]:
  the spawn draws of calls 1 and 2 of ordinal i (scenario_ref.agent_draws): origin gate oe, destination point di, offsets ud;
  candidates = gates g of cur's class (>= 0), g != oe, u[g][c] finite, c the cell floor((p - origin) / cell) in float32;
  untouched when p is NaN, c is outside the grid, cur is outside 0..G-1 or in no class, there is no candidate, or u[cur][c]
  is finite and <= commit;
  best = the candidate of least u (lowest gate on a tie); switch iff u[cur][c] is not finite or u[best][c] + margin < u[cur][c];
  on a switch d' = entries[best][di] + ud spawn_offset, waypoints[q][i] = d', exit_idx[q][i] = nearest_entry(d') for
  q = f .. 1, dest[i] = d'.
At t < 1 or (t - 1) % every != 0 nothing happens."""
import numpy as np

import scenario_ref

f32 = np.float32


def cells(metres, cell):
    """a law's margin or commit in cell units, divided in float32 as the host does"""
    with np.errstate(over='ignore'):
        return f32(f32(metres) / f32(cell))


def gate_class(classes, G):
    out = np.full(G, -1, np.int32)
    for k, c in enumerate(classes):
        out[list(c)] = k
    return out


def cell_of(p, x0, y0, cell, gx, gy):
    """(cx, cy) of nav_direction's cell formula, or None for a NaN position or a cell outside the grid"""
    if np.isnan(p).any():
        return None
    with np.errstate(over='ignore', invalid='ignore'):
        fcx = np.floor(f32(f32(p[0] - f32(x0)) / f32(cell)))
        fcy = np.floor(f32(f32(p[1] - f32(y0)) / f32(cell)))
    if not (0 <= fcx < gx and 0 <= fcy < gy):
        return None
    return int(fcx), int(fcy)


def decide(u, c, cls, cur, oe, margin, commit):
    """the gate slot bound for `cur` at cell c = (cx, cy) switches to, or None (steps 2-4)"""
    G = u.shape[0]
    if not 0 <= cur < G or cls[cur] < 0:
        return None
    col = u[:, c[1], c[0]].astype(f32)
    cand = [g for g in range(G) if cls[g] == cls[cur] and g != oe and np.isfinite(col[g])]
    if not cand:
        return None
    ucur = col[cur]
    if np.isfinite(ucur) and ucur <= f32(commit):
        return None
    best = min(cand, key=lambda g: (col[g], g))
    if best == cur:
        return None
    with np.errstate(over='ignore'):
        if not np.isfinite(ucur) or f32(col[best] + f32(margin)) < ucur:
            return best
    return None


def choose(state, u, x0, y0, cell, classes, margin, commit, every, t, seed, entries, spawn_offset):
    """-> (the new state, switched (cap) int32: 1 where the slot switched).  classes: gate_class(...)'s array."""
    s = {k: np.array(v) for k, v in state.items()}
    cap = s['p'].shape[0]
    switched = np.zeros(cap, np.int32)
    t, every = int(t), int(every)
    if t < 1 or (t - 1) % every != 0:
        return s, switched
    u = np.asarray(u, f32)
    G, gy, gx = u.shape
    entries = np.asarray(entries, f32)
    E, P = entries.shape[:2]
    n = min(int(s['n']), cap)
    if n == 0:
        return s, switched
    dr = scenario_ref.agent_draws(seed, np.arange(n), E, P)
    cls = np.asarray(classes, np.int32)
    for i in range(n):
        f = int(s['flag'][i])
        if s['mask'][i] == 0 or not 0 <= f < 2:
            continue
        c = cell_of(s['p'][i], x0, y0, cell, gx, gy)
        if c is None:
            continue
        best = decide(u, c, cls, int(s['exit_idx'][f, i]), int(dr['oe'][i]), margin, commit)
        if best is None:
            continue
        d = (entries[best, dr['di'][i]] + dr['ud'][i] * f32(spawn_offset)).astype(f32)
        ex = int(scenario_ref.nearest_entry(d[None], entries)[0])
        for q in range(f, 2):
            s['waypoints'][q, i] = d
            s['exit_idx'][q, i] = ex
        s['dest'][i] = d
        switched[i] = 1
    return s, switched
