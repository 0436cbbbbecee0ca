"""The exit choice's test states, built on the host in numpy and shared by tests/test_navchoice.py (properties of the
restatement) and tests/test_navchoice_gpu.py (the kernel against it).  One state per size holds every case of the rule: each
case has a cell of its own whose column of u is written by hand, so what decides is exact by construction."""
import functools

import numpy as np

import nav_ref
import navchoice_ref as REF

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)
CELL, X0, Y0 = 0.5, -1.0, 2.0
SPAWN_OFFSET = 0.8
P_POINTS = 5
D_ROWS = 3                                                      # one row more than the rule touches
MARGIN, COMMIT, EVERY = 0.75, 1.0, 8                             # metres, metres, frames: 1.5 and 2 cells, exact in float32
T_ON, T_OFF = 9, 8                                               # (t - 1) % 8 == 0, and not
GRIDS = {'row': (40, 1), 'ushape': (33, 34), 'big': (65, 65)}    # (gx, gy)
CASES = ('cur_unreachable', 'all_unreachable', 'equal', 'at_margin', 'ulp_below_margin', 'inside_commit', 'nan_position',
         'outside', 'mask0', 'retired', 'flag1', 'origin_nearest', 'cur_classless', 'tie_lowest', 'far_better')
BACKGROUND = 4                                                   # slots of random cells and gates between two rounds of CASES


def classes_of(G):
    """G = 3: gates 0 and 2 are one class, gate 1 is in none.  G = 64: 0..31 and 32..62, gate 63 in none."""
    return [[0, 2]] if G == 3 else [list(range(0, 32)), list(range(32, 63))]


@functools.lru_cache(maxsize=None)
def grid_case(grid, G):
    """blocked (gy, gx), goal (G, gy, gx), the solved field u (G, gy, gx) float32, entries (G, P, 2) float32, the free cells"""
    gx, gy = GRIDS[grid]
    if grid == 'ushape':
        blocked = nav_ref.u_shape_case()[0]
    else:
        blocked = np.zeros((gy, gx), np.uint8)
    free = [(x, y) for y in range(gy) for x in range(gx) if not blocked[y, x]]
    goal = np.zeros((G, gy, gx), np.uint8)
    entries = np.zeros((G, P_POINTS, 2), f32)
    for g in range(G):
        x, y = free[(g * 7919 + 3) % len(free)]
        goal[g, y, x] = 1
        for j in range(P_POINTS):
            entries[g, j] = (f32(X0) + f32(x + 0.1 + 0.2 * j) * f32(CELL), f32(Y0) + f32(y + 0.5) * f32(CELL))
    u, _ = nav_ref.solve(blocked, goal)
    return blocked, goal, u, entries, free


def centre(x, y, fx=0.5, fy=0.5):
    return np.array([f32(X0) + f32(x + fx) * f32(CELL), f32(Y0) + f32(y + fy) * f32(CELL)], f32)


def build(cap, members, G, grid, seeds=None):
    """-> dict: states (a list of per-member state dicts), u (members, G, gy, gx), entries, classes (G) int32, seeds, case (members,
    cap) the case index of each slot (-1: background), oe (members, cap)"""
    import scenario_ref
    blocked, goal, u0, entries, free = grid_case(grid, G)
    gx, gy = GRIDS[grid]
    seeds = list(range(11, 11 + members)) if seeds is None else seeds
    cls = REF.gate_class(classes_of(G), G)
    C = classes_of(G)[0]
    cur0, best0, lone = C[0], C[-1], (1 if G == 3 else 63)
    margin, commit = REF.cells(MARGIN, CELL), REF.cells(COMMIT, CELL)
    rng = np.random.default_rng(1000 * cap + 10 * G + members + len(grid))
    # a cell per case, spread over the free cells
    cells = {name: free[(k * 37 + 5) % len(free)] for k, name in enumerate(CASES)}
    assert len(set(cells.values())) == len(CASES)
    u = np.stack([(u0 * f32(1 + 0.5 * m)).astype(f32) for m in range(members)])
    for m in range(members):                                     # members disagree on which gate of a class is nearer
        u[m, best0] = (u[m, best0] * f32(1 + m)).astype(f32)

    def column(name, values, others=f32(60)):
        """u[:, :, cell of `name`] for every member: `others` + g on the gates not named"""
        x, y = cells[name]
        for g in range(G):
            u[:, g, y, x] = values.get(g, f32(others + g) if np.isfinite(others) else others)
    column('cur_unreachable', {cur0: INF, best0: f32(5)})
    column('all_unreachable', {}, others=INF)
    column('equal', {cur0: f32(7), best0: f32(7)})
    column('at_margin', {cur0: f32(f32(3) + margin), best0: f32(3)})
    column('ulp_below_margin', {cur0: np.nextafter(f32(f32(3) + margin), INF), best0: f32(3)})
    column('inside_commit', {cur0: commit, best0: f32(0.25)})
    column('flag1', {cur0: f32(30), best0: f32(4)})
    column('origin_nearest', {cur0: f32(30), best0: f32(4)})     # (the slot's own origin gate is written below)
    column('cur_classless', {lone: f32(40), cur0: f32(2), best0: f32(1)})
    column('tie_lowest', {cur0: f32(30), best0: f32(4), (C[1] if len(C) > 2 else best0): f32(4)})
    column('far_better', {cur0: f32(30), best0: f32(4)})
    for name in ('nan_position', 'outside', 'mask0', 'retired'):
        column(name, {cur0: f32(30), best0: f32(4)})
    states, case, oes = [], np.full((members, cap), -1, np.int64), []
    used = set(cells.values())
    spare = [c for c in free[::-1] if c not in used][:8]         # origin_nearest's cells, one per origin gate met
    own = {}
    n = cap - 2 if cap > 2 else cap                              # the last two slots have not been spawned yet
    period = len(CASES) + BACKGROUND
    for m in range(members):
        dr = scenario_ref.agent_draws(seeds[m], np.arange(cap), G, P_POINTS)
        oe = dr['oe']
        s = dict(p=np.zeros((cap, 2), f32), dest=rng.uniform(0, 9, (cap, 2)).astype(f32), flag=np.zeros(cap, np.int32),
                 mask=np.ones(cap, f32), waypoints=np.full((D_ROWS, cap, 2), NAN, f32),
                 exit_idx=np.zeros((D_ROWS, cap), np.int32), n=n)
        s['waypoints'][:2] = rng.uniform(0, 9, (2, cap, 2)).astype(f32)
        for i in range(cap):
            k = (i + m) % period
            if k >= len(CASES):                                  # background: a random free cell, gate and flag
                x, y = free[int(rng.integers(len(free)))]
                s['p'][i] = centre(x, y, *rng.uniform(0.1, 0.9, 2))
                s['flag'][i] = int(rng.integers(2))
                s['exit_idx'][:, i] = rng.integers(0, G, D_ROWS)
                continue
            name = CASES[k]
            case[m, i] = k
            x, y = cells[name]
            s['p'][i] = centre(x, y, *rng.uniform(0.1, 0.9, 2))
            s['exit_idx'][:, i] = cur0
            if name == 'nan_position':
                s['p'][i, int(rng.integers(2))] = NAN
            elif name == 'outside':
                s['p'][i] = centre(*[(-1, 0), (gx, 0), (0, -1), (0, gy)][i % 4])
            elif name == 'mask0':
                s['mask'][i] = 0
            elif name == 'retired':
                s['mask'][i], s['flag'][i] = 0, 2
                s['p'][i] = s['dest'][i] = NAN
            elif name == 'flag1':
                s['flag'][i] = 1
                s['exit_idx'][0, i] = lone                       # row 0 is the past: not read, not written
            elif name == 'cur_classless':
                s['exit_idx'][:, i] = lone
            elif name == 'origin_nearest' and cls[oe[i]] == cls[cur0] and oe[i] != cur0:
                # a cell per origin gate (while spare cells last) whose column reads lowest at that gate: the nearest gate of
                # the class is the one the agent came in through, and it is not a candidate
                g = int(oe[i])
                if g not in own and spare:
                    own[g] = spare.pop()
                    x, y = own[g]
                    for q in range(G):
                        u[:, q, y, x] = f32(60 + q)
                    u[:, cur0, y, x], u[:, best0, y, x] = f32(30), f32(4)
                    u[:, g, y, x] = f32(0.5)
                if g in own:
                    s['p'][i] = centre(*own[g], *rng.uniform(0.1, 0.9, 2))
        states.append(s)
        oes.append(oe)
    return dict(states=states, u=u, entries=entries, classes=cls, seeds=seeds, case=case, oe=np.stack(oes), blocked=blocked,
                goal=goal, gx=gx, gy=gy, G=G, n=n, margin=margin, commit=commit)


def expected(case, t=T_ON, classes=None, margin=None, shared_field=False):
    """the restatement on every member of build()'s case -> (states, switched (members, cap))"""
    out, sw = [], []
    for m, s in enumerate(case['states']):
        new, w = REF.choose(s, case['u'][0 if shared_field else m], X0, Y0, CELL, case['classes'] if classes is None else classes,
                            case['margin'] if margin is None else margin, case['commit'], EVERY, t, case['seeds'][m],
                            case['entries'], SPAWN_OFFSET)
        out.append(new)
        sw.append(w)
    return out, np.stack(sw)
