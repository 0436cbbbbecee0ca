"""Float64 numpy restatement of the track statistics (piml_amd.trackstats), with the items whose
classification float32 cannot be trusted to share flagged as ambiguous.

Everything is computed twice, in float64 (over the float32 inputs and the float32 options) and in float32 numpy (the
formulas as written, each operation rounded: IEEE subtraction, product, sum, division and square root are correctly
rounded in numpy and on the device alike, and rint rounds to even as llrintf does).  An item is a lag pair (two mover
steps L apart), an MSD pair (two participating frames L apart), an acceleration item (two consecutive steps) or a step.
With tol(x) = max(1e-5 |x|, 1e-5), in float64:
  a step is ambiguous when its speed l / dt lies within tol of v_min or the two runs disagree on `mover`;
  a lag pair (both steps movers in either run, or ambiguous) is ambiguous when one of its steps is;
  an MSD pair is ambiguous when sqrt(d2) lies within tol of d_max or the runs disagree on near / far;
  an acceleration item is ambiguous when a lies within tol of a bin edge k acc_bin (1 <= k <= acc_bins; a >= 0 in both runs,
  so 0 is no edge) or the runs disagree on its bin or on a < acc_bin acc_bins.

track_stats returns the float64 outputs, the float32 run's (`f32`) and per output a tolerance of the same shape (`tol`).
The per-item bounds, with eps = 2^-24 the relative error of one float32 operation and ulp(x) the float32 spacing at x
(eps |x| <= ulp(x)); e(u) is the rounding error of the float32 subtraction that forms a component of u, which is 0 when the
difference is exact (coordinates on a common grid) and is taken as |u32 - u64| of the two runs, the device performing the
same IEEE subtraction:
  ac_n, msd_n, msd_far, acc: the ambiguous items touching the entry (for acc: the float64 bin, its two neighbours and the
      float32 bin);
  ac_sum: 2 per unambiguous pair -- u carries eps, l = sqrt(ux^2 + uy^2) 2.5 eps, h = u / l 4.5 eps per component, the dot
      product of two headings an absolute error below 11 eps, 0.66 units at Q = 2^20, and the two roundings to integers
      move the difference to at most 1 -- plus Q + 2 per ambiguous pair (|h.h'| <= 1 + 11 eps);
  msd_sum: per unambiguous pair 1 + 4 ulp(d2 Q) -- d carries eps, its square 3 eps, the sum 4 eps; rounding to integers
      adds 1 -- plus d_max^2 Q (1 + 1e-4) per ambiguous pair;
  acc_sum: per unambiguous item 1 + 4 ulp(a Q) + (sum of e(u) over the four components) Q / dt^2 -- with exact u the
      difference u' - u is exact too, the squares and their sum carry 2 eps, the root 2 eps, the two divisions 4 eps --
      plus acc_bin acc_bins Q per ambiguous item;
  trk_path: per step 1 + 2 ulp(l Q) + (e(ux) + e(uy)) Q -- squares and sum 2 eps, root 2 eps; trk_net: the same bound on
      p(last) - p(first);
  trk_frames, trk_steps, trk_first, trk_last: exact.
n_items counts the float64 items, n_ambiguous the ambiguous ones; f32_deviation the largest |float64 - float32| term over
the unambiguous items."""
import numpy as np

LAG_ROWS = ('ac_n', 'ac_sum', 'msd_n', 'msd_sum', 'msd_far')
TRACK_ROWS = ('trk_frames', 'trk_steps', 'trk_first', 'trk_last', 'trk_path', 'trk_net')
OUTPUTS = LAG_ROWS + ('acc', 'acc_sum') + TRACK_ROWS
EXACT = ('trk_frames', 'trk_steps', 'trk_first', 'trk_last')
REL = 1e-5
Q = 1 << 20
MAX_COORD = 65536.0


def _tol(x):
    return np.maximum(REL * np.abs(x), REL)


def _near(x, level):
    return np.abs(x - level) <= _tol(level)


def _ulp(x):
    """the float32 spacing at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def participants(p, m):
    with np.errstate(invalid='ignore'):
        return (m == 1) & (np.abs(p) < MAX_COORD).all(-1)


def _rint(x):
    return np.rint(np.where(np.isfinite(x), x, 0)).astype(np.int64)


def _member(p32, part, o, dt):
    """every per-item quantity of one member in dtype dt: p32 (T', n, 2) float32, part (T', n) bool"""
    f = lambda x: np.asarray(x, np.float32).astype(dt)
    step, vmin, dmax, abin = f(o['dt']), f(o['v_min']), f(o['d_max']), f(o['acc_bin'])
    AB, NL = o['acc_bins'], o['n_lags']
    top = abin * dt(AB)
    p = np.where(part[..., None], p32, 0).astype(dt)
    Tp = p.shape[0]
    r = {}
    with np.errstate(all='ignore'):
        ex = part[:-1] & part[1:]                                 # (T' - 1, n): step t exists
        u = p[1:] - p[:-1]
        l = np.sqrt(u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1])
        speed = l / step
        mover = ex & (speed >= vmin)
        h = np.where(mover[..., None], u / np.where(mover, l, 1)[..., None], 0).astype(dt)
        r.update(ex=ex, u=u, l=l, speed=speed, mover=mover, h=h, lq=_rint(l * dt(Q)))
        # acceleration items
        ex2 = ex[:-1] & ex[1:]
        g = u[1:] - u[:-1]
        a = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) / step / step
        qb = np.floor(a / abin)
        r.update(ex2=ex2, a=a, bin=np.where(qb < AB, qb, AB).astype(np.int64), summed=a < top, aq=_rint(a * dt(Q)))
        # per lag
        r['lags'] = []
        for L in range(1, NL + 1):
            if L >= Tp:
                r['lags'].append(None)
                continue
            both = part[:-L] & part[L:]
            d = p[L:] - p[:-L]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
            dist = np.sqrt(d2)
            near = both & (dist < dmax)
            e = dict(both=both, d2=d2, dist=dist, near=near, d2q=_rint(np.where(near, d2, 0) * dt(Q)))
            if L < Tp - 1:
                mv = mover[:-L] & mover[L:]
                c = h[:-L, :, 0] * h[L:, :, 0] + h[:-L, :, 1] * h[L:, :, 1]
                e.update(mv=mv, cq=_rint(np.where(mv, c, 0) * dt(Q)))
            r['lags'].append(e)
    return r


def track_stats(P, M, dt=0.08, v_min=0.1, n_lags=128, d_max=64.0, acc_bin=0.25, acc_bins=40, frames=None, n_active=None):
    P, M = np.asarray(P, np.float32), np.asarray(M, np.float32)
    if P.ndim == 3:
        P, M = P[None], M[None]
    S, T, N = M.shape
    t0, t1 = frames if frames is not None else (0, T)
    Tp, NL, AB = t1 - t0, int(n_lags), int(acc_bins)
    o = dict(dt=dt, v_min=v_min, n_lags=NL, d_max=d_max, acc_bin=acc_bin, acc_bins=AB)
    z = lambda *shape: np.zeros(shape, np.int64)

    def blank():
        d = {k: z(S, NL) for k in LAG_ROWS}
        d.update(acc=z(S, AB + 1), acc_sum=z(S))
        d.update({k: z(S, N) for k in TRACK_ROWS})
        d['trk_first'] -= 1
        d['trk_last'] -= 1
        return d
    out, f32, tol = blank(), blank(), blank()
    tol['trk_first'] += 1
    tol['trk_last'] += 1
    step64, vm64, dmax64, abin64 = (np.float64(np.float32(x)) for x in (dt, v_min, d_max, acc_bin))
    n_items = n_amb = 0
    worst = dict(ac_sum=0, msd_sum=0, acc_sum=0, trk_path=0)
    kinds = dict(lag=[0, 0], msd=[0, 0], acc=[0, 0], step=[0, 0])
    for s in range(S):
        bound = N if n_active is None else min(max(int(n_active[s]), 0), N)
        if bound == 0 or Tp == 0:
            continue
        p32, m = P[s, t0:t1, :bound], M[s, t0:t1, :bound]
        part = participants(p32, m)
        e, g = _member(p32, part, o, np.float64), _member(p32, part, o, np.float32)
        # track rows
        frames_n = part.sum(0)
        has = frames_n > 0
        first = np.where(has, part.argmax(0), -1)
        last = np.where(has, Tp - 1 - part[::-1].argmax(0), -1)
        cols = np.arange(bound)
        pf, pl = p32[np.maximum(first, 0), cols], p32[np.maximum(last, 0), cols]
        for res, dst, dtp in ((e, out, np.float64), (g, f32, np.float32)):
            dst['trk_frames'][s, :bound], dst['trk_first'][s, :bound], dst['trk_last'][s, :bound] = frames_n, first, last
            dst['trk_steps'][s, :bound] = res['ex'].sum(0)
            dst['trk_path'][s, :bound] = np.where(res['ex'], res['lq'], 0).sum(0)
            with np.errstate(all='ignore'):
                d = np.where((frames_n >= 2)[:, None], pl.astype(dtp) - pf.astype(dtp), 0)
                res['net_d'] = d
                res['net'] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) * dtp(Q)
            dst['trk_net'][s, :bound] = _rint(res['net'])
        ex = e['ex']
        eu = np.abs(g['u'].astype(np.float64) - e['u']).sum(-1)               # e(ux) + e(uy) per step
        t_path = np.where(ex, 1 + 2 * _ulp(e['l'] * Q) + eu * Q, 0)
        tol['trk_path'][s, :bound] = np.ceil(t_path.sum(0)).astype(np.int64)
        en = np.abs(g['net_d'].astype(np.float64) - e['net_d']).sum(-1)
        tol['trk_net'][s, :bound] = np.ceil(np.where(frames_n >= 2, 1 + 2 * _ulp(e['net']) + en * Q, 0)).astype(np.int64)
        worst['trk_path'] = max(worst['trk_path'], int(np.abs(e['lq'] - g['lq'])[ex].max(initial=0)))
        # steps
        amb_step = ex & (_near(e['speed'], vm64) | (e['mover'] != g['mover']))
        kinds['step'][0] += int(ex.sum())
        kinds['step'][1] += int(amb_step.sum())
        # acceleration items
        ex2 = e['ex2']
        if ex2.size:
            k_edge = np.rint(e['a'] / abin64)
            amb_a = ex2 & ((e['bin'] != g['bin']) | (e['summed'] != g['summed'])
                           | ((k_edge >= 1) & (k_edge <= AB) & (np.abs(e['a'] - k_edge * abin64) <= _tol(e['a']))))
            for res, dst in ((e, out), (g, f32)):
                np.add.at(dst['acc'][s], res['bin'][ex2], 1)
                dst['acc_sum'][s] = int(res['aq'][ex2 & res['summed']].sum())
            sure = ex2 & ~amb_a & e['summed']
            eu4 = eu[1:] + eu[:-1]
            t_acc = np.where(sure, 1 + 4 * _ulp(e['a'] * Q) + eu4 * Q / (step64 * step64) * (1 + 1e-6), 0).sum()
            top_q = float(np.float32(acc_bin)) * AB * Q
            tol['acc_sum'][s] = int(np.ceil(t_acc + amb_a.sum() * (top_q * (1 + 1e-4) + 1)))
            for b64, b32 in zip(e['bin'][amb_a].tolist(), g['bin'][amb_a].tolist()):
                for x in {b64 - 1, b64, b64 + 1, b32}:
                    if 0 <= x <= AB:
                        tol['acc'][s, x] += 1
            worst['acc_sum'] = max(worst['acc_sum'], int(np.abs(e['aq'] - g['aq'])[sure & g['summed']].max(initial=0)))
            kinds['acc'][0] += int(ex2.sum())
            kinds['acc'][1] += int(amb_a.sum())
        # lags
        for L in range(1, NL + 1):
            le, lg = e['lags'][L - 1], g['lags'][L - 1]
            if le is None:
                continue
            both = le['both']
            amb_m = both & (_near(le['dist'], dmax64) | (le['near'] != lg['near']))
            for res, dst in ((le, out), (lg, f32)):
                dst['msd_n'][s, L - 1] = int(res['near'].sum())
                dst['msd_far'][s, L - 1] = int((both & ~res['near']).sum())
                dst['msd_sum'][s, L - 1] = int(res['d2q'][res['near']].sum())
            sure = le['near'] & ~amb_m
            n_am = int(amb_m.sum())
            tol['msd_n'][s, L - 1] = tol['msd_far'][s, L - 1] = n_am
            t_msd = np.where(sure, 1 + 4 * _ulp(le['d2'] * Q), 0).sum() + n_am * (dmax64 * dmax64 * Q * (1 + 1e-4) + 1)
            tol['msd_sum'][s, L - 1] = int(np.ceil(t_msd))
            worst['msd_sum'] = max(worst['msd_sum'], int(np.abs(le['d2q'] - lg['d2q'])[sure & lg['near']].max(initial=0)))
            kinds['msd'][0] += int(both.sum())
            kinds['msd'][1] += n_am
            if 'mv' not in le:
                continue
            cand = (e['mover'] | g['mover'] | amb_step)
            cand = cand[:-L] & cand[L:]
            amb_p = cand & (amb_step[:-L] | amb_step[L:])
            for res, dst in ((le, out), (lg, f32)):
                dst['ac_n'][s, L - 1] = int(res['mv'].sum())
                dst['ac_sum'][s, L - 1] = int(res['cq'][res['mv']].sum())
            sure = le['mv'] & ~amb_p
            n_ap = int(amb_p.sum())
            tol['ac_n'][s, L - 1] = n_ap
            tol['ac_sum'][s, L - 1] = 2 * int(sure.sum()) + (Q + 2) * n_ap
            worst['ac_sum'] = max(worst['ac_sum'], int(np.abs(le['cq'] - lg['cq'])[sure & lg['mv']].max(initial=0)))
            kinds['lag'][0] += int(le['mv'].sum())
            kinds['lag'][1] += n_ap
    n_items = sum(v[0] for v in kinds.values())
    n_amb = sum(v[1] for v in kinds.values())
    out['tol'], out['f32'] = tol, f32
    out['n_items'], out['n_ambiguous'], out['kinds'] = n_items, n_amb, kinds
    out['f32_deviation'] = worst
    return out


def check(got, want, label=''):
    """every output of `got` (dict or object of int arrays) equals want's within want's tolerance, and the float32 run's bit
    for bit when no item is ambiguous; returns the largest deviation per output as (against float64, against float32)"""
    dev = {}
    get = lambda k: np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
    for k in OUTPUTS:
        g, w = get(k), want[k]
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        dev[k] = (int(np.abs(g - w).max(initial=0)), int(np.abs(g - want['f32'][k]).max(initial=0)))
    print(f'[trackstats] {label}: largest deviation (float64, float32 run) ' + ', '.join(f'{k} {v}' for k, v in dev.items()))
    for k in OUTPUTS:
        g = get(k)
        bad = np.abs(g - want[k]) > want['tol'][k]
        assert not bad.any(), (label, k, np.argwhere(bad)[:5].tolist(), g[bad][:5].tolist(), want[k][bad][:5].tolist(),
                               want['tol'][k][bad][:5].tolist())
        if want['n_ambiguous'] == 0:
            assert np.array_equal(g, want['f32'][k]), (label, k, 'differs from the float32 run')
    return dev


def random_tracks(S, T, N, seed, dt=0.08, centred=False):
    """Smooth random walks, one presence interval per slot: heading noise 0.08 rad per frame, speeds from Gamma(4, 0.3) m/s
    with one agent in ten near rest (0 .. 0.2 m/s, either side of v_min), 3 % holes inside the interval, and a sprinkle of
    NaN and infinite positions, coordinates of 65536 and masks of 0.5.  Positions lie on the grid of 2^-14 m around
    (768, 640), where float32 holds them and all their differences exactly; `centred` starts them within 10 m of the origin
    without the grid instead, so that differences round.  Returns P (S, T, N, 2) and M (S, T, N) float32."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, max(T - 1, 1), (S, N))
    b = np.minimum(a + 2 + rng.integers(0, T, (S, N)), T)
    throughout = rng.random((S, N)) < 0.15
    a, b = np.where(throughout, 0, a), np.where(throughout, T, b)
    t = np.arange(T)[None, :, None]
    M = ((t >= a[:, None, :]) & (t < b[:, None, :])).astype(np.float32)
    M[rng.random((S, T, N)) < 0.03] = 0.0
    speed = rng.gamma(4.0, 0.3, (S, 1, N))
    slow = rng.random((S, 1, N)) < 0.1
    speed = np.where(slow, 0.2 * rng.random((S, 1, N)), speed) * (1.0 + 0.05 * rng.normal(0.0, 1.0, (S, T, N)))
    theta = rng.random((S, 1, N)) * 2 * np.pi + np.cumsum(rng.normal(0.0, 0.08, (S, T, N)), 1)
    u = np.stack([np.cos(theta), np.sin(theta)], -1) * (speed * dt)[..., None]
    start = rng.random((S, 1, N, 2)) * 20.0 - 10.0
    x = start + np.cumsum(u, 1)
    if centred:
        P = x.astype(np.float32)
    else:
        P = (np.array([768.0, 640.0]) + np.rint(x * 16384.0) / 16384.0).astype(np.float32)
    r = rng.random((S, T, N))
    P[r < 0.004] = np.nan
    P[(r >= 0.004) & (r < 0.006), 0] = np.inf
    P[(r >= 0.006) & (r < 0.008), 1] = -65536.0
    M[(r >= 0.008) & (r < 0.012)] = 0.5
    return P, M
