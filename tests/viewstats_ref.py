"""Float64 numpy restatement of the heading-frame pair statistics (piml_amd.viewstats), with the pairs and
agents whose classification float32 cannot be trusted to share flagged as ambiguous.

Everything is computed twice, in float64 (over the float32 inputs and the float32 options) and in float32 numpy (the
formulas as written, each operation rounded).  With tol(x) = max(1e-5 |x|, 1e-5), in float64:
  an agent is speed-ambiguous when its speed lies within tol of v_min or the two runs disagree on `mover`, box-ambiguous when
  a coordinate lies within tol of a box edge;
  a pair (focal i in either run, participant j != i, evaluated in either run or with r within tol of r_max) is ambiguous
  when the runs disagree on it (evaluated, class, cell), when r lies within tol of r_max, when a + X or l + X lies within
  tol of a multiple of the cell (for a cell on the map or one cell outside it: further out no edge can change a count),
  when j moves and q lies within tol of +-cos_same, when i or j is speed-ambiguous or i box-ambiguous;
  a focal agent's nearest neighbour is ambiguous when the runner-up's r lies within tol of the minimum, when the winner (of
  either run) is an ambiguous pair or the runs disagree on it, when an ambiguous pair lies within tol of the minimum, or
  when the agent is speed- or box-ambiguous;
  its front gap is ambiguous when a source of the corridor widened by tol has |l| within tol of the corridor or a within
  tol of 0 or is evaluated in one run only or has r within tol of r_max, when the minimum lies within tol of a bin edge,
  when the runner-up lies within tol of it and falls in another bin, when the runs disagree on the bin, or when the agent is
  speed- or box-ambiguous.

view_stats returns the float64 outputs, the float32 run's (`f32`) and per output a tolerance of the same shape (`tol`):
  focal: the speed- or box-ambiguous focal agents of the lag; pairs: the ambiguous pairs of the lag;
  map: the ambiguous pairs touching the cell, in every class (their float64 cell, its eight neighbours, their float32
      cell -- flowstats_ref._touch in two dimensions);
  nn_map: the ambiguous agents touching the cell (the cells of both runs' winners and of the runner-up with their
      neighbours, and the open last bin);
  front_gap: the ambiguous agents touching the bin (the float64 bin, its two neighbours, the float32 bin, the bins with
      and without the doubtful sources, the open last bin);
  front_speed: 2 per unambiguous agent of the bin + the own |llrint(sp Q)| of every ambiguous agent touching it.
n_pairs counts the float64 evaluated pairs, n_ambiguous the ambiguous ones among the candidates."""
import numpy as np

OUTPUTS = ('focal', 'pairs', 'map', 'nn_map', 'front_gap', 'front_speed')
REL = 1e-5
Q = 1 << 20
MAX_SPEED = 1024.0
COS_SAME = np.float32(np.cos(np.pi / 4))


def _tol(x):
    return np.maximum(REL * np.abs(x), REL)


def _near(x, level):
    return np.abs(x - level) <= _tol(level)


def participants(p, v, m):
    with np.errstate(invalid='ignore'):
        return (m == 1) & np.isfinite(p).all(-1) & (np.abs(v) < MAX_SPEED).all(-1)


def agents(v, v_min, dt):
    """per agent in dtype dt: speed, mover, heading (NaN where not a mover)"""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    vx, vy, vm = f(v[:, 0]), f(v[:, 1]), f(v_min)
    with np.errstate(all='ignore'):
        s = np.sqrt(vx * vx + vy * vy)
        mover = s >= vm
        hx, hy = np.where(mover, vx / s, np.nan), np.where(mover, vy / s, np.nan)
    return dict(s=s, mover=mover, hx=hx.astype(dt), hy=hy.astype(dt))


def classify(pi, ai, pj, aj, same, o, dt):
    """Per pair (focal rows x participant columns) in dtype dt: ev (evaluated), r, a, l, ux = a + X, uy = l + X, the cell
    (cx, cy as floats), inmap, cidx (cy G + cx, G G outside), q = h_i.h_j and the class."""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    cell, X, cs, G = f(o['cell']), f(o['X']), f(o['cos_same']), o['G']
    with np.errstate(all='ignore'):
        dx = f(pj[None, :, 0]) - f(pi[:, None, 0])
        dy = f(pj[None, :, 1]) - f(pi[:, None, 1])
        r = np.sqrt(dx * dx + dy * dy)
        ev = ~same
        if o['r_max'] is not None:
            ev = ev & ~(r >= f(o['r_max']))
        hx, hy = ai['hx'][:, None], ai['hy'][:, None]
        a = dx * hx + dy * hy
        l = dy * hx - dx * hy
        ux, uy = a + X, l + X
        cx, cy = np.floor(ux / cell), np.floor(uy / cell)
        inmap = ev & (cx >= 0) & (cx < G) & (cy >= 0) & (cy < G)
        cidx = np.where(inmap, cy * G + cx, G * G).astype(np.int64)
        q = hx * aj['hx'][None, :] + hy * aj['hy'][None, :]
        cls = np.where(~aj['mover'][None, :], 0, np.where(q >= cs, 1, np.where(q <= -cs, 2, 3))).astype(np.int64)
        cls = np.broadcast_to(cls, r.shape)
    return dict(ev=ev, r=r, a=a, l=l, ux=ux, uy=uy, cx=cx, cy=cy, inmap=inmap, cidx=cidx, q=q, cls=cls)


def _hood(cx, cy, G):
    """the map indices of cell (cx, cy) and its eight neighbours, and G G when one of them lies outside the map"""
    out = set()
    if not (np.isfinite(cx) and np.isfinite(cy)):
        return {G * G}
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            x, y = int(cx) + a, int(cy) + b
            out.add(y * G + x if 0 <= x < G and 0 <= y < G else G * G)
    return out


def _bin(a, gb, GB):
    """floor(a / gap_bin) clipped to the open last bin"""
    with np.errstate(all='ignore'):
        b = np.floor(a / gb)
    return np.where(b < GB, b, GB).astype(np.int64)


def view_stats(P, V, M, lags=(64, 128, 192), v_min=0.1, cell=0.25, half=12, cos_same=COS_SAME, r_max=None, corridor=0.4,
               gap_bin=0.1, gap_bins=60, box=None, frames=None, n_active=None):
    P, V, M = (np.asarray(x, np.float32) for x in (P, V, M))
    if P.ndim == 3:
        P, V, M = P[None], V[None], M[None]
    S, T, N = M.shape
    t0, t1 = frames if frames is not None else (0, T)
    all_lags = (0,) + tuple(int(x) for x in lags)
    K1, G, GB = len(all_lags), 2 * int(half), int(gap_bins)
    GG = G * G
    o = dict(cell=np.float32(cell), X=np.float32(np.float32(cell) * np.float32(half)), cos_same=np.float32(cos_same), G=G,
             r_max=None if r_max is None else np.float32(r_max))
    bx = None if box is None else [np.float32(v) for v in box]
    z = lambda *shape: np.zeros(shape, np.int64)
    blank = lambda: dict(focal=z(S, K1), pairs=z(S, K1), map=z(S, K1, 4, G, G), nn_map=z(S, GG + 1), front_gap=z(S, GB + 1),
                         front_speed=z(S, GB))
    out, f32, tol = blank(), blank(), blank()
    vm64, c64, cs64, corr64, gb64 = (np.float64(np.float32(x)) for x in (v_min, cell, cos_same, corridor, gap_bin))
    rmax64 = None if r_max is None else np.float64(np.float32(r_max))
    n_pairs = n_amb = 0
    runs = ((np.float64, out), (np.float32, f32))
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        for k, lag in enumerate(all_lags):
            for t in range(t0, t1 - lag):
                p, v, m = P[s, t, :bound], V[s, t, :bound], M[s, t, :bound]
                pj_, vj_, mj_ = P[s, t + lag, :bound], V[s, t + lag, :bound], M[s, t + lag, :bound]
                inbox = participants(p, v, m)
                if bx is not None:
                    inbox &= (bx[0] <= p[:, 0]) & (p[:, 0] < bx[1]) & (bx[2] <= p[:, 1]) & (p[:, 1] < bx[3])
                all_i = {dt: agents(v, v_min, dt) for dt, _ in runs}
                fi = np.nonzero(inbox & (all_i[np.float64]['mover'] | all_i[np.float32]['mover']))[0]
                jj = np.nonzero(participants(pj_, vj_, mj_))[0]
                if not len(fi):
                    continue
                same = fi[:, None] == jj[None, :]
                A = {dt: ({key: val[fi] for key, val in all_i[dt].items()}, agents(vj_[jj], v_min, dt)) for dt, _ in runs}
                e = classify(p[fi], A[np.float64][0], pj_[jj], A[np.float64][1], same, o, np.float64)
                g = classify(p[fi], A[np.float32][0], pj_[jj], A[np.float32][1], same, o, np.float32)
                foc = {np.float64: A[np.float64][0]['mover'], np.float32: A[np.float32][0]['mover']}
                spd_i = _near(A[np.float64][0]['s'], vm64) | (foc[np.float64] != foc[np.float32])
                spd_j = _near(A[np.float64][1]['s'], vm64) | (A[np.float64][1]['mover'] != A[np.float32][1]['mover'])
                box_i = np.zeros(len(fi), bool)
                if bx is not None:
                    pf = p[fi].astype(np.float64)
                    for q_, c in ((0, 0), (1, 0), (2, 1), (3, 1)):
                        box_i |= _near(pf[:, c], np.float64(bx[q_]))
                agent_amb = spd_i | box_i
                with np.errstate(all='ignore'):
                    near_rmax = np.zeros(same.shape, bool) if rmax64 is None else (~same & _near(e['r'], rmax64))
                    cand = ~same & (e['ev'] | g['ev'] | near_rmax)
                    near_map = (e['cx'] >= -1) & (e['cx'] <= G) & (e['cy'] >= -1) & (e['cy'] <= G)
                    edge = near_map & ((np.abs(e['ux'] - np.rint(e['ux'] / c64) * c64) <= _tol(e['ux']))
                                       | (np.abs(e['uy'] - np.rint(e['uy'] / c64) * c64) <= _tol(e['uy'])))
                    movers_j = (A[np.float64][1]['mover'] | A[np.float32][1]['mover'])[None, :]
                    q_amb = movers_j & (_near(e['q'], cs64) | _near(e['q'], -cs64))
                    ev_amb = cand & ((e['ev'] != g['ev']) | near_rmax)
                    amb = cand & (ev_amb | (e['cls'] != g['cls']) | (e['cidx'] != g['cidx']) | edge | q_amb
                                  | agent_amb[:, None] | spd_j[None, :])
                for (dt, dst), res in zip(runs, (e, g)):
                    rows = foc[dt]
                    dst['focal'][s, k] += int(rows.sum())
                    dst['pairs'][s, k] += int(res['ev'][rows].sum())
                    sel = res['inmap'] & rows[:, None]
                    np.add.at(dst['map'][s, k].reshape(-1), res['cls'][sel] * GG + res['cidx'][sel], 1)
                n_pairs += int(e['ev'][foc[np.float64]].sum())
                n_amb += int(amb.sum())
                tol['focal'][s, k] += int(agent_amb.sum())
                tol['pairs'][s, k] += int(amb.sum())
                tmap = tol['map'][s, k].reshape(4, GG)
                for a_, b_ in zip(*np.nonzero(amb)):
                    cells = (_hood(e['cx'][a_, b_], e['cy'][a_, b_], G) if near_map[a_, b_] else set()) | {int(g['cidx'][a_, b_])}
                    for c in cells:
                        if c < GG:
                            tmap[:, c] += 1
                if lag != 0:
                    continue
                # the nearest neighbour and the front gap of every focal agent
                res_nn, res_gap = {}, {}
                for (dt, dst), res in zip(runs, (e, g)):
                    rows = foc[dt]
                    r_ev = np.where(res['ev'], res['r'], np.inf)
                    j1 = r_ev.argmin(1) if r_ev.shape[1] else np.zeros(len(fi), np.int64)
                    has = np.isfinite(r_ev.min(1, initial=np.inf))
                    nn = np.where(has, res['cidx'][np.arange(len(fi)), j1] if r_ev.shape[1] else GG, GG)
                    np.add.at(dst['nn_map'][s], nn[rows], 1)
                    with np.errstate(all='ignore'):
                        front = res['ev'] & (res['a'] > 0) & (np.abs(res['l']) < dt(np.float32(corridor)))
                        am = np.where(front, res['a'], np.inf).min(1, initial=np.inf)
                        gbin = _bin(am, dt(np.float32(gap_bin)), GB)
                        qs = np.rint(A[dt][0]['s'] * dt(Q))
                    qs = np.where(rows, qs, 0).astype(np.int64)
                    np.add.at(dst['front_gap'][s], gbin[rows], 1)
                    ok = rows & (gbin < GB)
                    np.add.at(dst['front_speed'][s], gbin[ok], qs[ok])
                    res_nn[dt] = (j1, has, nn, r_ev)
                    res_gap[dt] = (front, am, gbin, qs)
                (j64, has64, nn64, r64), (j32, has32, nn32, _) = res_nn[np.float64], res_nn[np.float32]
                (front64, am64, bin64, qs64), (_, _, bin32, qs32) = res_gap[np.float64], res_gap[np.float32]
                rows_any = foc[np.float64] | foc[np.float32]
                idx = np.arange(len(fi))
                ncol = r64.shape[1]
                if ncol >= 2:
                    part = np.partition(r64, 1, axis=1)
                    m1, m2 = part[:, 0], part[:, 1]
                    order2 = np.argsort(r64, axis=1, kind='stable')[:, 1]
                else:
                    m1 = r64.min(1, initial=np.inf)
                    m2, order2 = np.full(len(fi), np.inf), np.zeros(len(fi), np.int64)
                with np.errstate(all='ignore'):
                    runner = np.isfinite(m2) & (m2 - m1 <= _tol(m1))
                    close_amb = (amb & (e['r'] <= (m1 + _tol(m1))[:, None])).any(1) if ncol else np.zeros(len(fi), bool)
                win_amb = (amb[idx, j64] | amb[idx, j32]) if ncol else np.zeros(len(fi), bool)
                nn_amb = rows_any & (agent_amb | runner | win_amb | close_amb | (has64 != has32) | (j64 != j32) | (nn64 != nn32))
                for a_ in np.nonzero(nn_amb)[0]:
                    cells = {GG, int(nn32[a_])}
                    if ncol:
                        cells |= _hood(e['cx'][a_, j64[a_]], e['cy'][a_, j64[a_]], G)
                        cells |= _hood(e['cx'][a_, j32[a_]], e['cy'][a_, j32[a_]], G)
                        cells |= _hood(e['cx'][a_, order2[a_]], e['cy'][a_, order2[a_]], G)
                    for c in cells:
                        tol['nn_map'][s, c] += 1
                with np.errstate(all='ignore'):
                    wide = cand & (e['a'] > -REL) & (np.abs(e['l']) < corr64 + _tol(corr64))
                    risky = wide & (_near(np.abs(e['l']), corr64) | _near(e['a'], 0.0) | ev_amb)
                    k_edge = np.rint(am64 / gb64)
                    edge_bin = np.isfinite(am64) & (k_edge <= GB) & (np.abs(am64 - k_edge * gb64) <= _tol(am64))
                    a_front = np.where(front64, e['a'], np.inf)
                    a2 = np.partition(a_front, 1, axis=1)[:, 1] if ncol >= 2 else np.full(len(fi), np.inf)
                    runner_g = np.isfinite(a2) & (a2 - am64 <= _tol(am64)) & (_bin(a2, gb64, GB) != bin64)
                    sure_min = np.where(front64 & ~risky, e['a'], np.inf).min(1, initial=np.inf)
                    wide_min = np.where(wide | front64, np.maximum(e['a'], 0.0), np.inf).min(1, initial=np.inf)
                gap_amb = rows_any & (agent_amb | risky.any(1) | edge_bin | runner_g | (bin64 != bin32))
                sure_rows = foc[np.float64] & ~gap_amb & (bin64 < GB)
                np.add.at(tol['front_speed'][s], bin64[sure_rows], 2)
                for a_ in np.nonzero(gap_amb)[0]:
                    bins = {int(bin64[a_]) - 1, int(bin64[a_]), int(bin64[a_]) + 1, int(bin32[a_]), GB,
                            int(_bin(sure_min[a_], gb64, GB)), int(_bin(wide_min[a_], gb64, GB))}
                    own = max(abs(int(qs64[a_])), abs(int(qs32[a_])),
                              abs(int(np.rint(np.float64(A[np.float64][0]['s'][a_]) * Q))))
                    for b in bins:
                        if 0 <= b <= GB:
                            tol['front_gap'][s, b] += 1
                            if b < GB:
                                tol['front_speed'][s, b] += own
    out['tol'], out['f32'] = tol, f32
    out['n_pairs'], out['n_ambiguous'] = n_pairs, n_amb
    return out


def check(got, want, label=''):
    """every output of `got` (dict or object of int arrays) equals want's within want's tolerance; returns the largest
    deviation per output as (against float64, against the float32 run)"""
    dev = {}
    for k in OUTPUTS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = want[k]
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        dev[k] = (int(np.abs(g - w).max(initial=0)), int(np.abs(g - want['f32'][k]).max(initial=0)))
    print(f'[viewstats] {label}: largest deviation (float64, float32 run) ' + ', '.join(f'{k} {v}' for k, v in dev.items()))
    for k in dev:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        bad = np.abs(g - want[k]) > want['tol'][k]
        assert not bad.any(), (label, k, np.argwhere(bad)[:5].tolist(), g[bad][:5].tolist(), want[k][bad][:5].tolist(),
                               want['tol'][k][bad][:5].tolist())
    return dev
