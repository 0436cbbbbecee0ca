"""Numpy restatement of the group statistics (piml_amd.groupstats): both device passes and the host half, with the
pair-frames whose classification float32 cannot be trusted to share flagged as ambiguous.

Everything is computed twice: in float32 numpy (the formulas as written, each operation rounded: IEEE subtraction, product,
sum, division and square root are correctly rounded in numpy and on the device alike, and rint rounds to even as llrintf
does) and in float64 over the same float32 inputs and the same float32 thresholds.  An item is a pair-frame (i, j, t): both
steps exist at t.  It is ambiguous, by linestats_ref's rule, when the two runs disagree on any of its four predicates
(distance, velocity difference, the two speeds) or, where either run finds it together, on a bin it would fall into (the
distance bin, skipped or not, the formation bin) -- whether or not its pair turns out to be a link.

group_stats returns the float32 run's outputs (device and host arrays), the float64 run's under 'f64', n_items,
n_ambiguous and the ambiguous items per member ('amb').  check() asserts that a result equals the float32 run bit for bit.

planted_tracks generates walkers with planted pairs, triples and a chain (uniform random positions per frame hold no
persistent pair and would leave every output vacuous); analytic_scene is a hand-counted scene on multiples of 1/8 m."""
import math

import numpy as np

Q = 1 << 20
MAX_COORD = 65536.0
G_MAX = 8
SHARE_UNIT = 1024
PAIR_ROWS = ('trk_steps', 'trk_path', 'pairs', 'together')
MEMBER_ROWS = ('dist', 'dist_sum', 'abreast', 'abreast_skipped', 'link_frames')
HOST_ROWS = ('candidates', 'links', 'group_id', 'size_tracks', 'size_path', 'size_steps')
OUTPUTS = ('edges', 'n_edges') + PAIR_ROWS + MEMBER_ROWS + HOST_ROWS


def thresholds(dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8):
    """(r2, dv2, vm2) float32, each made once in float64 and rounded once; min_frames; share_q"""
    r2 = np.float32(float(radius) ** 2)
    dv2 = np.float32((float(dv_max) * float(dt)) ** 2)
    vm2 = np.float32((float(v_min) * float(dt)) ** 2)
    return r2, dv2, vm2, max(1, math.ceil(float(min_time) / float(dt))), int(round(float(share) * SHARE_UNIT))


def participants(p, m):
    with np.errstate(invalid='ignore'):
        return (m == 1) & (np.abs(p) < MAX_COORD).all(-1)


def _rint(x):
    return np.rint(x).astype(np.int64)


def host_rows(edges, trk_steps, trk_path, min_frames, share_q, g_max=G_MAX):
    """the host half restated: plain loops and a flood fill over the links of each member"""
    edges = np.asarray(edges, np.int64).reshape(-1, 5)
    S, N = trk_steps.shape
    z = lambda *shape: np.zeros(shape, np.int64)
    out = dict(candidates=z(S), links=z(S), group_id=np.full((S, N), -1, np.int32), size_tracks=z(S, g_max + 1),
               size_path=z(S, g_max + 1), size_steps=z(S, g_max + 1))
    for s in range(S):
        nbr = [[] for _ in range(N)]
        for m, i, j, co, near in edges.tolist():
            if m != s:
                continue
            out['candidates'][s] += 1
            if near * SHARE_UNIT >= share_q * co:
                out['links'][s] += 1
                nbr[i].append(j)
                nbr[j].append(i)
        seen = [False] * N
        for n in range(N):
            if seen[n] or trk_steps[s, n] < min_frames:
                continue
            comp, todo = [], [n]
            seen[n] = True
            while todo:
                x = todo.pop()
                comp.append(x)
                for y in nbr[x]:
                    if not seen[y]:
                        seen[y] = True
                        todo.append(y)
            assert all(trk_steps[s, x] >= min_frames for x in comp)      # every end of a candidate is eligible
            k = min(len(comp), g_max)
            for x in comp:
                out['group_id'][s, x] = min(comp)
                out['size_tracks'][s, k] += 1
                out['size_path'][s, k] += trk_path[s, x]
                out['size_steps'][s, k] += trk_steps[s, x]
    return out


def _pass(dt, p, u, ex, i, tt, th, r_bin, RB, AB):
    """every per-item quantity of focal i against the partners j > i over the focal's steps tt, in dtype dt"""
    r2, dv2, vm2 = (dt(x) for x in th)
    both = ex[tt][:, i + 1:]
    e = p[tt][:, i + 1:] - p[tt, i][:, None]
    ui, uj = u[tt, i][:, None], u[tt][:, i + 1:]
    g = uj - ui
    with np.errstate(all='ignore'):
        e2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
        g2 = g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]
        ui2 = ui[..., 0] * ui[..., 0] + ui[..., 1] * ui[..., 1]
        uj2 = uj[..., 0] * uj[..., 0] + uj[..., 1] * uj[..., 1]
        preds = (e2 < r2, g2 < dv2, np.broadcast_to(ui2 >= vm2, e2.shape), uj2 >= vm2)
        tog = both & preds[0] & preds[1] & preds[2] & preds[3]
        d = np.sqrt(e2)
        qb = np.floor(d / dt(np.float32(r_bin)))
        w = ui + uj
        w2 = w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]
        skip = (e2 == 0) | (w2 == 0)
        c = np.abs(e[..., 0] * w[..., 0] + e[..., 1] * w[..., 1]) / (np.sqrt(e2) * np.sqrt(w2))
        qa = np.floor(np.where(skip, 0, c) * dt(AB))
        dq = _rint(np.where(both, d, 0) * dt(Q))
    return dict(both=both, preds=preds, tog=tog, dbin=np.where(qb < RB, qb, RB).astype(np.int64), dq=dq, skip=skip,
                abin=np.where(qa < AB - 1, qa, AB - 1).astype(np.int64))


def group_stats(P, M, dt=0.08, radius=2.0, dv_max=0.5, v_min=0.1, min_time=2.0, share=0.8, r_bin=0.1, r_bins=20, a_bins=10,
                frames=None, n_active=None, g_max=G_MAX):
    P, M = np.asarray(P, np.float32), np.asarray(M, np.float32)
    if P.ndim == 3:
        P, M = P[None], M[None]
    S, T, N = M.shape
    t0, t1 = frames if frames is not None else (0, T)
    Tp, RB, AB = t1 - t0, int(r_bins), int(a_bins)
    r2, dv2, vm2, min_frames, share_q = thresholds(dt, radius, dv_max, v_min, min_time, share)
    z = lambda *shape: np.zeros(shape, np.int64)

    def blank():
        return dict(edges=[], n_edges=z(S), trk_steps=z(S, N), trk_path=z(S, N), pairs=z(S), together=z(S), dist=z(S, RB + 1),
                    dist_sum=z(S), abreast=z(S, AB), abreast_skipped=z(S), link_frames=z(S))
    runs = (blank(), blank())
    amb = z(S)
    n_items = 0
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        if bound == 0 or Tp < 2:
            continue
        p32, m = P[s, t0:t1, :bound], M[s, t0:t1, :bound]
        part = participants(p32, m)
        ex = part[:-1] & part[1:]
        state = []
        for dst, dtp in zip(runs, (np.float32, np.float64)):
            p = np.where(part[..., None], p32, 0).astype(dtp)
            u = p[1:] - p[:-1]
            with np.errstate(all='ignore'):
                length = np.sqrt(u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1])
            dst['trk_steps'][s, :bound] = ex.sum(0)
            dst['trk_path'][s, :bound] = np.where(ex, _rint(np.where(ex, length, 0) * dtp(Q)), 0).sum(0)
            state.append((dtp, p[:-1], u))
        for i in range(bound - 1):
            tt = np.nonzero(ex[:, i])[0]
            if tt.size == 0:
                continue
            res = [_pass(dtp, p, u, ex, i, tt, (r2, dv2, vm2), r_bin, RB, AB) for dtp, p, u in state]
            for dst, r in zip(runs, res):
                co, near = r['both'].sum(0), r['tog'].sum(0)
                dst['pairs'][s] += int(co.sum())
                dst['together'][s] += int(near.sum())
                for k in np.nonzero(near >= min_frames)[0]:
                    dst['edges'].append((s, i, i + 1 + int(k), int(co[k]), int(near[k])))
                    if int(near[k]) * SHARE_UNIT >= share_q * int(co[k]):
                        on = r['tog'][:, k]
                        dst['link_frames'][s] += int(on.sum())
                        np.add.at(dst['dist'][s], r['dbin'][on, k], 1)
                        dst['dist_sum'][s] += int(r['dq'][on, k].sum())
                        sk = r['skip'][on, k]
                        dst['abreast_skipped'][s] += int(sk.sum())
                        np.add.at(dst['abreast'][s], r['abin'][on, k][~sk], 1)
            a, b = res
            n_items += int(a['both'].sum())
            differ = np.zeros(a['both'].shape, bool)
            for x, y in zip(a['preds'], b['preds']):
                differ |= x != y
            either = a['tog'] | b['tog']
            differ |= either & ((a['dbin'] != b['dbin']) | (a['skip'] != b['skip']) | (~a['skip'] & (a['abin'] != b['abin'])))
            amb[s] += int((a['both'] & differ).sum())
    for dst in runs:
        dst['edges'] = np.asarray(sorted(dst['edges']), np.int64).reshape(-1, 5)
        dst['n_edges'] = np.bincount(dst['edges'][:, 0], minlength=S).astype(np.int64)
        dst.update(host_rows(dst['edges'], dst['trk_steps'], dst['trk_path'], min_frames, share_q, g_max))
    out = dict(runs[0])
    out.update(f64=runs[1], n_items=n_items, n_ambiguous=int(amb.sum()), amb=amb, min_frames=min_frames, share_q=share_q)
    return out


def check(stats, want, label=''):
    """every device and host array of `stats` (dict or object of int arrays) equals want's float32 run bit for bit.  Returns
    per array the largest deviation from the float64 run."""
    get = lambda k: np.asarray(stats[k] if isinstance(stats, dict) else getattr(stats, k))
    dev = {}
    for k in OUTPUTS:
        g, w = get(k), want[k]
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        assert np.array_equal(g, w), (label, k, 'differs from the float32 run', np.argwhere(g != w)[:5].tolist())
        f = want['f64'][k]
        dev[k] = int(np.abs(g - f).max(initial=0)) if f.shape == g.shape else -1
    print(f'[groupstats] {label}: equal to the float32 run; largest deviation from the float64 run '
          + ', '.join(f'{k} {v}' for k, v in dev.items()))
    return dev


KINDS = ('triple', 'pair', 'chain', 'short', 'lowshare', 'pair', 'triple', 'pair')


def planted_tracks(S, T, N, seed, dt=0.08):
    """P (S, T, N, 2), M (S, T, N) float32 and per member the planted groups [(kind, slots)]: straight walkers (0.8 - 1.5 m/s)
    with small per-frame noise, staggered entry and exit frames, gaps of absent frames in the middle of some tracks, NaN and
    infinite coordinates and masks of 0.5.  About a third of the slots (all of them when N < 8) are planted: a follower
    copies its leader's displacement plus noise at an offset of 0.5 - 1.5 m ('pair'; 0.5 - 1 m in a 'triple').  'short': the
    follower is there for a few frames only (less than min_time); 'lowshare': it walks along for 55 % of its frames and then
    turns away (together for less than `share` of the common frames); 'chain': two followers 1.4 m ahead of and behind
    the leader, each linked to it and 2.8 m from each other."""
    rng = np.random.default_rng(seed)
    side = max(math.sqrt(N / 0.05), 20.0)
    P = np.zeros((S, T, N, 2))
    M = np.zeros((S, T, N), np.float32)
    plans = []
    rich = T >= 8

    def span():
        q = T // 4 if rich and N >= 8 else 0                # a small case is one group, there from the first frame to the last
        return int(rng.integers(0, q + 1)), T - int(rng.integers(0, q + 1))

    def put(s, n, start, disp, t_in, t_out):
        P[s, :, n] = start + np.concatenate([np.zeros((1, 2)), np.cumsum(disp, 0)])[:T]
        M[s, t_in:t_out, n] = 1.0

    def leader_disp():
        ang = rng.random() * 2 * math.pi
        v = rng.uniform(0.8, 1.5)
        d = np.array([math.cos(ang), math.sin(ang)]) * v * dt
        return d, d + rng.normal(0.0, 0.002, (T, 2))

    for s in range(S):
        slots = list(rng.permutation(N)) if N >= 8 else list(range(N))
        budget = N // 3 if N >= 8 else N
        plan, k = [], 0
        while budget >= 2:
            kind = KINDS[k % len(KINDS)] if N >= 8 else ('triple' if budget >= 3 else 'pair')
            k += 1
            size = 3 if kind in ('triple', 'chain') else 2
            if size > budget:
                kind, size = 'pair', 2
            mine = [int(slots.pop()) for _ in range(size)]
            budget -= size
            plan.append((kind, mine))
            mean, disp = leader_disp()
            start = rng.random(2) * side
            t_in, t_out = span()
            put(s, mine[0], start, disp, t_in, t_out)
            ahead = mean / np.linalg.norm(mean)
            for f, n in enumerate(mine[1:]):
                if kind == 'chain':
                    off = ahead * (1.4 if f == 0 else -1.4)
                else:
                    ang = rng.random() * 2 * math.pi
                    off = np.array([math.cos(ang), math.sin(ang)]) * rng.uniform(0.5, 1.0 if kind == 'triple' else 1.5)
                fd = disp + rng.normal(0.0, 0.002, (T, 2))
                f_in = min(t_in + int(rng.integers(0, 2)), t_out - 1) if rich else t_in
                f_out = t_out
                if kind == 'short':
                    f_out = min(f_in + max(2, T // 8), t_out)
                if kind == 'lowshare':
                    turn = f_in + int(0.55 * (t_out - f_in))
                    fd[turn:] = fd[turn:][:, ::-1] * np.array([-1.0, 1.0])     # a quarter turn
                put(s, n, start + off, fd, f_in, f_out)
        for n in slots:                                                        # the single walkers
            _, disp = leader_disp()
            put(s, int(n), rng.random(2) * side, disp, *span())
        plans.append(plan)
    if rich:
        for s in range(S):
            for n in range(N):
                t = np.nonzero(M[s, :, n])[0]
                if t.size >= 6 and rng.random() < 0.15:                        # a gap in the middle
                    mid = int(t[t.size // 2])
                    M[s, mid:mid + int(rng.integers(1, 4)), n] = 0.0
        r = rng.random((S, T, N))
        P[r < 0.005] = np.nan
        P[(r >= 0.005) & (r < 0.008), 0] = np.inf
        M[(r >= 0.008) & (r < 0.013) & (M == 1)] = 0.5
    with np.errstate(over='ignore'):
        return P.astype(np.float32), M, plans


def analytic_scene():
    """A hand-counted scene on multiples of 1/8 m (exact in float32 and float64): P (1, 40, 6, 2), M, the options and the hand
    counts.  dt = 0.08 s, every walker moves 0.125 m per frame.  Agents 0 and 1 walk along +x side by side 1 m apart, agent
    2 walks 1.5 m behind agent 0 in file (sqrt(3.25) m from agent 1); agent 3 walks the other way 0.5 m beside agent 0's
    path and passes it; agent 4 walks alone 50 m away and agent 5 stands still 0.5 m from agent 4's path.  One group,
    {0, 1, 2}, with three links; r_bin = 0.125 m puts 1 m, 1.5 m and sqrt(3.25) m into bins 8, 12 and 14."""
    T, N = 40, 6
    t = np.arange(T, dtype=np.float64)
    P = np.zeros((1, T, N, 2))
    M = np.ones((1, T, N), np.float32)
    x, y = P[0, :, :, 0], P[0, :, :, 1]
    x[:, 0], y[:, 0] = 5.0 + 0.125 * t, 10.0
    x[:, 1], y[:, 1] = 5.0 + 0.125 * t, 11.0
    x[:, 2], y[:, 2] = 3.5 + 0.125 * t, 10.0
    x[:, 3], y[:, 3] = 10.0 - 0.125 * t, 9.5
    x[:, 4], y[:, 4] = 5.0 + 0.125 * t, 60.0
    x[:, 5], y[:, 5] = 7.0, 60.5
    kw = dict(dt=0.08, r_bin=0.125, r_bins=20, a_bins=10)
    n = T - 1
    root = int(np.rint(np.sqrt(np.float32(3.25)) * np.float32(Q)))
    z = lambda *shape: np.zeros(shape, np.int64)
    step = Q // 8
    h = dict(edges=np.array([[0, 0, 1, n, n], [0, 0, 2, n, n], [0, 1, 2, n, n]]), n_edges=np.array([3]),
             trk_steps=np.full((1, N), n), trk_path=np.array([[n * step] * 5 + [0]]), pairs=np.array([15 * n]),
             together=np.array([3 * n]), dist=z(1, 21), dist_sum=np.array([n * (Q + 3 * Q // 2 + root)]), abreast=z(1, 10),
             abreast_skipped=z(1), link_frames=np.array([3 * n]), candidates=np.array([3]), links=np.array([3]),
             group_id=np.array([[0, 0, 0, 3, 4, 5]], np.int32), size_tracks=z(1, G_MAX + 1), size_path=z(1, G_MAX + 1),
             size_steps=z(1, G_MAX + 1))
    h['dist'][0, [8, 12, 14]] = n
    h['abreast'][0, [0, 8, 9]] = n                       # 0-1 side by side, 1-2 at |cos| = 1.5 / sqrt(3.25) = 0.83, 0-2 in file
    h['size_tracks'][0, [1, 3]] = 3
    h['size_path'][0, 1], h['size_path'][0, 3] = 2 * n * step, 3 * n * step
    h['size_steps'][0, [1, 3]] = 3 * n
    return P.astype(np.float32), M, kw, h
