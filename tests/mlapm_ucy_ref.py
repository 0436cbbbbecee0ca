"""Float64 yardstick for the UCY variant of MLAPM.step (mlapm.py:10-58 with coll.unsqueeze(-1)) and the scenes that put
its two-phase kernels under pressure.  Plain torch + numpy; no GPU needed (step64 takes a device for large N).

The UCY law has three piecewise-constant factors: the collision flag (mlapm.py:43-47), the field of view (:27) and the
sign of the rotation (:47-48).  The flag is a discrete decision the kernels take in the reference's exact float32
operations, so `flags` takes it the same way, and reports which pairs are `decidable` -- the same answer in float64 with
the thresholds moved by DELTA either way.  View and rotation sign are taken in float64; `kink_margin` measures how far a
scene keeps every pair from their zero crossings, and the scene builders redraw the few agents that come closer than KINK
(a float32 evaluation of either expression is within 1e-6 of its scale, see kink_margin)."""
import collections
import math

import numpy as np
import torch

DELTA = 1e-4          # decidability: thresholds 2R (1 -+ DELTA), tmin window (0, 1) shrunk / widened by DELTA
KINK = 1e-5           # smallest |cos| a scene keeps between (v_i, r_ij) and between (e_i, r_ij) off a right angle / parallel
TILE = 2048           # agents per LDS tile of the kernels (kMlTile)

UCY_LAW = dict(tau=5 / 6, A=10.67, B=-3.33, C=0.5, theta=20.0)      # _LAWS['UCY'] of the pairwise tests
JUMP_LAW = dict(tau=0.9, A=3.0, B=-1.0, C=3.0, theta=20.0)          # g = exp(3 - r): a flagged pair is ~ 10-20 x its g = 1 term

Step64 = collections.namedtuple('Step64', 'action m grads flag')


def _t32(x):
    return torch.tensor(np.array(x, dtype=np.float32))


def flags(p, v, radius, delta=DELTA):
    """(flag, decidable), both (N, N) bool numpy, [focal, source].  flag: mlapm.py:43-47 in float32 torch operations on
    the CPU, as written there.  decidable: the float64 predicate on the same float32 inputs agrees with flag both with
    (thresholds 2R (1 - delta), tmin in (delta, 1 - delta)) and with (2R (1 + delta), tmin in (-delta, 1 + delta)); the
    predicate is monotone in both, so these two bracket every mixed setting.  The diagonal is set decidable (excluded)."""
    p, v = _t32(p), _t32(v)
    two_r32 = radius * 2                                      # (a Python scalar: compared in the tensors' float32)
    dp, dv = p[None, :, :] - p[:, None, :], v[None, :, :] - v[:, None, :]        # [focal, source]
    rw, ww, rr = (dp * dv).sum(-1), (dv * dv).sum(-1), (dp * dp).sum(-1)         # x x' + y y': two products, one sum
    coll = (dp.norm(dim=-1) < two_r32) | ((dp + dv).norm(dim=-1) < two_r32)      # now, and after one unit of time
    tmin, dmin = -rw / ww, (rr - rw * rw / ww).sqrt()                            # closest approach: when, how near
    coll = coll | ((tmin > 0) & (tmin < 1) & (dmin < two_r32))
    p, v = p.double(), v.double()
    vr = p.view(1, -1, 2) - p.view(-1, 1, 2)
    vv = v.view(1, -1, 2) - v.view(-1, 1, 2)
    two_r = float(np.float32(radius) * np.float32(2))        # the float32 threshold both sides compare against
    d0, d1 = vr.norm(dim=-1), (vr + vv).norm(dim=-1)
    rw, ww, rr = (vr * vv).sum(-1), (vv * vv).sum(-1), (vr * vr).sum(-1)
    tmin = -rw / ww
    dmin = (rr - rw ** 2 / ww).clamp_min(0).sqrt()            # (NaN for ww == 0 stays NaN: compares false)
    decidable = torch.ones_like(coll)
    for s in (-1.0, 1.0):
        thr = two_r * (1 + s * delta)
        c = (d0 < thr) | (d1 < thr) | ((tmin > -s * delta) & (tmin < 1 + s * delta) & (dmin < thr))
        decidable &= c == coll
    decidable.fill_diagonal_(True)
    return coll.numpy(), decidable.numpy()


def candidates(p, v, radius):
    """The kernels' conservative filter in float64: [focal, source] True where the pair is NOT certainly far, i.e. not
    (a > 0 and a^2 > 1e-6 |r|^2 + 1e-6 + (2R)^2) with a = |r| - |w|.  The diagonal is a candidate (a = 0)."""
    p, v = _t32(p).double(), _t32(v).double()
    r = (p.view(1, -1, 2) - p.view(-1, 1, 2)).norm(dim=-1)
    w = (v.view(1, -1, 2) - v.view(-1, 1, 2)).norm(dim=-1)
    a = r - w
    two_r = float(np.float32(radius) * np.float32(2))
    return (~((a > 0) & (a * a > 1e-6 * r * r + 1e-6 + two_r ** 2))).numpy()


def _kinks(p, v, dest):
    """|cos| of the angle between v_i and r_ij (view, :27) and |sin| of the angle between e_i and r_ij (rotation sign,
    :47), [focal, source], float64; pairs where the expression is exactly zero on both sides (i == j, coincident agents,
    a focal agent at rest) are set to 1."""
    p, v, dest = _t32(p).double(), _t32(v).double(), _t32(dest).double()
    vr = p.view(1, -1, 2) - p.view(-1, 1, 2)
    r = vr.norm(dim=-1)
    e = torch.nn.functional.normalize(dest - p, dim=-1)
    sp = v.norm(dim=-1)[:, None]
    view = (v[:, None, :] * vr).sum(-1).abs() / (sp * r)
    sign = (vr[..., 0] * e[:, None, 1] - vr[..., 1] * e[:, None, 0]).abs() / r
    one = torch.ones_like(r)
    return torch.where((r > 0) & (sp > 0), view, one), torch.where(r > 0, sign, one)


def kink_margin(p, v, dest):
    """Smallest relative distance of any ordered pair from a zero crossing of the view test v_i . r_ij > 0 or of the
    rotation sign r_ij x e_i.  Float32 evaluates either as two products and one sum of numbers known to ~2 ulp (r_ij is a
    rounded difference, e_i a rounded quotient): below 1e-6 of |r| |v| resp. |r|.  A scene with a margin above KINK takes
    the same two decisions in float32 (fused or not) and float64."""
    view, sign = _kinks(p, v, dest)
    return float(torch.minimum(view.min(), sign.min()))


def step64(p, v, v0, dest, law, dt, radius, w=None, present=None, device='cpu'):
    """MLAPM.step, version UCY, in float64 on float32 inputs.  Returns Step64(action (N, 2), m (N,), grads, flag):
    m_i = |v_i| + dt (|desired force_i| + sum_j |term_ij|), the magnitude the forward error is measured against; grads
    (with an upstream w (N, 2)) the gradients of sum(action * w) on (p, v, v0, dest) by autograd -- the flag is a constant
    mask, view and the rotation sign carry none, as in the reference; flag as `flags` gives it.  present (N,) bool:
    the reference's host-side compaction (main_mlapm.py:18-36) -- only present agents are focal agents or sources; the rows
    of the others are NaN (forward only)."""
    p, v, dest = [np.asarray(x, dtype=np.float32) for x in (p, v, dest)]
    v0 = np.asarray(v0, dtype=np.float32).reshape(-1)
    N = p.shape[0]
    if present is not None:
        assert w is None, 'the gradient is defined for scenes without absent agents'
        idx = np.flatnonzero(np.asarray(present))
        sub = step64(p[idx], v[idx], v0[idx], dest[idx], law, dt, radius, device=device)
        action, m = np.full((N, 2), np.nan), np.full(N, np.nan)
        action[idx], m[idx] = sub.action, sub.m
        return Step64(action, m, None, sub.flag)
    flag = flags(p, v, radius)[0]
    P, V, V0, D = [torch.tensor(x, dtype=torch.float64, device=device, requires_grad=w is not None) for x in (p, v, v0, dest)]
    c = torch.as_tensor(flag, device=device).double()
    e = torch.nn.functional.normalize(D - P, dim=-1)
    want = (V0[:, None] * e - V) / law['tau']
    vr = P[None, :, :] - P[:, None, :]                                   # [focal, source]
    r = vr.norm(dim=-1)
    n = torch.nn.functional.normalize(vr, dim=-1)
    with torch.no_grad():
        view = ((V[:, None, :] * vr).sum(-1) > 0).double()
        cr = vr[..., 0] * e[:, None, 1] - vr[..., 1] * e[:, None, 0]
        th = torch.where(cr > 0, -1.0, 1.0) * (law['theta'] / 180 * math.pi)      # -sign(cr) theta, 0 -> +theta
        cs, sn = th.cos(), th.sin()
    gfac = view * law['A'] * torch.exp(law['B'] * r * c + law['C'] * c)
    direc = torch.stack([cs * n[..., 0] - sn * n[..., 1], sn * n[..., 0] + cs * n[..., 1]], dim=-1)
    force = want - (gfac[..., None] * direc).sum(dim=1)
    action = V + force * dt
    m = V.norm(dim=-1) + dt * (want.norm(dim=-1) + (gfac[..., None] * direc).norm(dim=-1).sum(dim=1))
    grads = None
    if w is not None:
        W = torch.as_tensor(np.asarray(w, dtype=np.float64), device=device)
        grads = [g.cpu().numpy() for g in torch.autograd.grad(action, [P, V, V0, D], W)]
    return Step64(action.detach().cpu().numpy(), m.detach().cpu().numpy(), grads, flag)


def step32(p, v, v0, dest, law, dt, radius):
    """The same law in float32 torch operations on the CPU (flag as `flags`): what a bar that a scene cannot meet is
    checked against before anything else."""
    P, V, D = _t32(p), _t32(v), _t32(dest)
    V0 = _t32(v0).reshape(-1)
    c = torch.as_tensor(flags(p, v, radius)[0]).float()
    e = torch.nn.functional.normalize(D - P, dim=-1)
    want = (V0[:, None] * e - V) / law['tau']
    vr = P[None, :, :] - P[:, None, :]
    r = vr.norm(dim=-1)
    n = torch.nn.functional.normalize(vr, dim=-1)
    view = ((V[:, None, :] * vr).sum(-1) > 0).float()
    cr = vr[..., 0] * e[:, None, 1] - vr[..., 1] * e[:, None, 0]
    th = torch.where(cr > 0, -1.0, 1.0) * (law['theta'] / 180 * math.pi)
    gfac = view * law['A'] * torch.exp(law['B'] * r * c + law['C'] * c)
    direc = torch.stack([th.cos() * n[..., 0] - th.sin() * n[..., 1], th.sin() * n[..., 0] + th.cos() * n[..., 1]], dim=-1)
    return (V + (want - (gfac[..., None] * direc).sum(dim=1)) * dt).numpy()


# ---- scenes: dicts of float32 arrays with synthetic_gc_scene's keys ----

def _scene(p, v, v0, dest, **extra):
    sc = dict(position=np.ascontiguousarray(p, dtype=np.float32), velocity=np.ascontiguousarray(v, dtype=np.float32),
              desired_speed=np.ascontiguousarray(v0, dtype=np.float32).reshape(-1, 1),
              destination=np.ascontiguousarray(dest, dtype=np.float32))
    sc.update(extra)
    return sc


def _unkink(p, v, dest, rng, redraw_view, rounds=50):
    """Redraws, in place and in a fixed order, what puts a focal agent within KINK of a zero crossing: its destination
    for the rotation sign (p + 10 randn again), and through redraw_view(i) whatever the scene may change for the view."""
    for _ in range(rounds):
        view, sign = _kinks(p, v, dest)
        bad_v = np.flatnonzero((view < KINK).any(1).numpy())
        bad_s = np.flatnonzero((sign < KINK).any(1).numpy())
        if not len(bad_v) and not len(bad_s):
            return
        for i in bad_s:
            dest[i] = p[i] + 10 * rng.standard_normal(2)
        for i in bad_v:
            redraw_view(i)
    raise AssertionError('a scene that keeps off the view / rotation-sign crossings was not found')


def _lattice(n, rng):
    """n points on a 5 m lattice, jittered by up to 0.5 m"""
    side = int(math.ceil(math.sqrt(n)))
    pts = np.array([(ix, iy) for iy in range(side) for ix in range(side)][:n], dtype=np.float64) * 5.0
    return pts + rng.uniform(-0.5, 0.5, size=(n, 2))


def clump_scene(N, lo, n, seed):
    """n agents (indices lo .. lo + n - 1) inside a disc of radius 0.27 m, at least 0.02 m apart, velocities
    (1.0, 0.3) + 0.3 randn: every pair of them is closer than 2R = 0.6, so each is a candidate of and flagged by every
    other.  The other N - n agents on a jittered 5 m lattice with velocities 0.8 randn; destinations p + 10 randn."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(max(N - n, 1))))
    centre = np.array([5.0 * (side // 2) + 2.5, 5.0 * (side // 2) - 2.5])      # the middle of a lattice cell
    clump = []
    while len(clump) < n:
        q = rng.uniform(-0.27, 0.27, size=2)
        if q @ q < 0.27 ** 2 and all((q - c) @ (q - c) >= 0.02 ** 2 for c in clump):
            clump.append(q)
    p = np.empty((N, 2))
    v = np.empty((N, 2))
    inside = np.zeros(N, bool)
    inside[lo:lo + n] = True
    p[inside] = centre + np.array(clump)
    v[inside] = np.array([1.0, 0.3]) + 0.3 * rng.standard_normal((n, 2))
    if N > n:
        p[~inside] = _lattice(N - n, rng)
        v[~inside] = 0.8 * rng.standard_normal((N - n, 2))
    dest = p + 10 * rng.standard_normal((N, 2))
    v0 = rng.uniform(0.8, 1.6, size=N)
    p, v, dest = [x.astype(np.float32) for x in (p, v, dest)]

    def redraw_view(i):
        v[i] = (np.array([1.0, 0.3]) + 0.3 * rng.standard_normal(2)) if inside[i] else 0.8 * rng.standard_normal(2)
    _unkink(p, v, dest, rng, redraw_view)
    return _scene(p, v, v0, dest, clump=inside)


def sparse_scene(N, drift=(0.0, 0.0)):
    """Agents on a jittered 5 m lattice, all with the velocity `drift`: w = 0 for every pair, no candidates.  At rest
    (the default) an agent sees nobody (view is v . r > 0) and the action is the desired-force step alone; with a drift
    every term is the g = 1 term."""
    rng = np.random.default_rng(N)
    p = _lattice(N, rng).astype(np.float32)
    v = np.tile(np.asarray(drift, dtype=np.float32), (N, 1))
    dest = (p + 10 * rng.standard_normal((N, 2))).astype(np.float32)
    v0 = rng.uniform(0.8, 1.6, size=N)

    def redraw_view(i):
        p[i] = np.round(p[i] / 5.0) * 5.0 + rng.uniform(-0.5, 0.5, size=2)
    _unkink(p, v, dest, rng, redraw_view)
    return _scene(p, v, v0, dest)


def boundary_scene(seed, radius=0.3, coincident=True):
    """Isolated pairs (agents 2k, 2k + 1), each just inside or just outside the boundary of the conservative filter, far
    from every other pair (asserted).  Returns the scene with `pairs`: a list of (i, j, kind, expected flag).
      head-on: w antiparallel to r, |r| - |w| = 2R (1 -+ 1e-3), |r| in {0.7, 5, 40, 300} -- inside is flagged by |r + w| < 2R,
               outside by nothing (tmin = |r| / |w| > 1);
      glancing: closest approach dmin = 2R (1 -+ 1e-3) at tmin in {0.05, 0.5, 0.95}, |r| in {1.5, 4, 10} (third clause only);
      w = 0 exactly: at rest and moving together, |r| = 0.5 (flagged by |r| < 2R) and 0.7 (tmin = -rw / 0: not flagged);
      coincident: d^2 = 0, different velocities (flagged; the term itself is zero; forward only -- coincident=False
                  puts the two 0.3 m apart instead).
    Both agents of a pair move (v = -+ w / 2), towards each other, so each sees the other."""
    rng = np.random.default_rng(seed)
    two_r = float(np.float32(radius) * np.float32(2))
    specs = []
    for rn in (0.7, 5.0, 40.0, 300.0):
        for s in (-1, 1):
            specs.append(('head-on', rn, s, None))
    for rn in (1.5, 4.0, 10.0):
        for t in (0.05, 0.5, 0.95):
            for s in (-1, 1):
                specs.append(('glancing', rn, s, t))
    for rn in (0.5, 0.7):
        specs.append(('rest', rn, 0, None))
        specs.append(('together', rn, 0, None))
    specs.append(('coincident', 0.0 if coincident else 0.3, 0, None))
    p, v, pairs, reach = [], [], [], []
    x = 0.0
    for k, (kind, rn, s, t) in enumerate(specs):
        ang = rng.uniform(0, 2 * math.pi)
        rhat = np.array([math.cos(ang), math.sin(ang)])
        perp = np.array([-rhat[1], rhat[0]])
        target = two_r * (1 + s * 1e-3)
        speed = {'head-on': (rn - target) / 2, 'rest': 0.0, 'together': 1.0, 'coincident': 1.0}.get(kind)
        if kind == 'glancing':
            speed = math.sqrt(rn ** 2 - target ** 2) / t / 2
        rch = rn / 2 + speed + 5.0                              # the pair stays within this of its centre, with room
        x += rch + (reach[-1] if reach else 0.0)
        reach.append(rch)
        centre = np.array([x, 3.0 * rng.standard_normal()])
        pi = (centre - rhat * rn / 2).astype(np.float32)
        pj = (centre + rhat * rn / 2).astype(np.float32)
        r = pj.astype(np.float64) - pi.astype(np.float64)       # what the float32 positions realise
        rl = float(np.linalg.norm(r))
        if kind == 'head-on':
            wv = -r / rl * (rl - target)
            vi, vj, expect = -wv / 2, wv / 2, s < 0
        elif kind == 'glancing':
            L = math.sqrt(rl ** 2 - target ** 2)
            u = (-L * r / rl + target * np.array([-r[1], r[0]]) / rl) / rl      # r . u = -L, closest approach at distance target
            wv = u * (L / t)
            vi, vj, expect = -wv / 2, wv / 2, s < 0
        elif kind == 'rest':
            vi, vj, expect = np.zeros(2), np.zeros(2), rn < two_r
        elif kind == 'together':
            vi = vj = 1.0 * (0.8 * rhat + 0.6 * perp)
            expect = rn < two_r
        else:
            vi, vj, expect = 1.0 * rhat, -0.7 * perp, True
        p += [pi, pj]
        v += [np.asarray(vi, dtype=np.float32), np.asarray(vj, dtype=np.float32)]
        pairs.append((2 * k, 2 * k + 1, kind, bool(expect)))
    p, v = np.array(p, dtype=np.float32), np.array(v, dtype=np.float32)
    N = len(p)
    dest = (p + 10 * rng.standard_normal((N, 2))).astype(np.float32)
    v0 = rng.uniform(0.8, 1.6, size=N)
    # every pair of agents that is not a constructed pair is far by a wide margin: (|r| - |w|)^2 above four times the filter's bound
    P, V = p.astype(np.float64), v.astype(np.float64)
    rr = np.linalg.norm(P[None] - P[:, None], axis=-1)
    a = rr - np.linalg.norm(V[None] - V[:, None], axis=-1)
    cross = np.ones((N, N), bool)
    for i, j, _, _ in pairs:
        cross[i, j] = cross[j, i] = False
    np.fill_diagonal(cross, False)
    assert (a[cross] > 0).all() and (a[cross] ** 2 > 4 * (1e-6 * rr[cross] ** 2 + 1e-6 + two_r ** 2)).all()

    def redraw_view(i):
        raise AssertionError(f'boundary_scene({seed}): agent {i} is on a view crossing; take another seed')
    _unkink(p, v, dest, rng, redraw_view)
    return _scene(p, v, v0, dest, pairs=pairs)


# ---- the cases of the GPU tests: name -> scene (built once per process; treat the arrays as read-only) ----
CLUMP_SHAPES = {'clump130': (130, 0, 130), 'clump200': (200, 0, 200), 'clump310': (310, 5, 300), 'clump700': (700, 300, 150),
                'clump2200': (2200, 1950, 200)}                 # (N, clump start, clump size)
CLUMP_SEED = 1
BOUNDARY_SEED = 1
CASES = tuple(CLUMP_SHAPES) + ('boundary', 'boundary_apart', 'sparse257', 'sparse257_drift')
_built = {}


def case(name):
    if name not in _built:
        if name in CLUMP_SHAPES:
            sc = clump_scene(*CLUMP_SHAPES[name], CLUMP_SEED)
        elif name.startswith('boundary'):
            sc = boundary_scene(BOUNDARY_SEED, coincident=name == 'boundary')
        else:
            sc = sparse_scene(257, drift=(0.9, 0.4) if name.endswith('drift') else (0.0, 0.0))
        for x in sc.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _built[name] = sc
    return _built[name]


def absent_mask(sc, seed=7):
    """10 % of the agents absent: index 0, the last index, a tenth of the clump (where the scene has one) and the rest
    drawn from the others."""
    N = sc['position'].shape[0]
    rng = np.random.default_rng(seed)
    gone = np.zeros(N, bool)
    gone[[0, N - 1]] = True
    clump = sc.get('clump')
    if clump is not None and clump.any() and not clump.all():
        idx = np.flatnonzero(clump)
        gone[rng.choice(idx, size=max(1, len(idx) // 10), replace=False)] = True
    rest = np.flatnonzero(~gone)
    gone[rng.choice(rest, size=max(0, N // 10 - int(gone.sum())), replace=False)] = True
    return gone
