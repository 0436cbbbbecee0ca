"""Float64 yardstick of the two MLAPM calibration kernels (piml_mlapm_fit_loss_grad, piml_mlapm_rollout_fit_loss_grad), the
scenes the form tests run them on, and editors that send a pack to the kernel form it would not take by itself.  CPU only.

The law is src/models/mlapm.py:10-58 restated in float64 under autograd (step64).  The discrete decisions -- the view
test, the rotation sign and the UCY collision flag -- are taken in float32, as the reference and the kernels take them;
everything smooth runs in float64.  tests/test_mlapm_fit_ref.py holds it against the reference's own autograd."""
import copy
import math
import types

import numpy as np
import torch

NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
UNUSED = {'raw': (3, 4, 5), 'GC': (), 'UCY': (4,)}           # the constants a variant's law does not hold
PRESENT, INJECTED, CARRIED = 1, 2, 4                         # pack_windows' flag bits


def decision_margin(p, v, ed, version, radius):
    """How far the nearest discrete decision of one step is from going the other way, in float64 and relative: |cos| of
    the angle between v_i and r_ij (view), |sin| of the angle between e_i and r_ij (rotation sign; not raw), and for UCY
    the collision flag's three criteria -- |r| against 2 radius, |r + w| against 2 radius, and t_min against 0 and 1 with
    d_min against 2 radius -- each counted only where the others leave the flag to it.  inf without a pair."""
    inf = torch.tensor(float('inf'), dtype=torch.float64)
    if p.shape[0] < 2:
        return float(inf)
    vr, vv = p[None] - p[:, None], v[None] - v[:, None]
    r = vr.norm(dim=-1)
    pair = ~torch.eye(p.shape[0], dtype=torch.bool) & (r > 0)
    sp = v.norm(dim=-1)[:, None]
    m = torch.where(pair & (sp > 0), torch.einsum('nk,nmk->nm', v, vr).abs() / (sp * r), inf).min()
    if version != 'raw':
        cr = vr[..., 0] * ed[:, None, 1] - vr[..., 1] * ed[:, None, 0]
        m = torch.minimum(m, torch.where(pair & (ed.norm(dim=-1)[:, None] > 0), cr.abs() / r, inf).min())
    if version == 'UCY':
        R2 = 2 * radius
        r1 = (vr + vv).norm(dim=-1)
        w2 = (vv * vv).sum(-1)
        tmin = -(vr * vv).sum(-1) / w2
        dmin = (r * r - (vr * vv).sum(-1) ** 2 / w2).clamp(min=0).sqrt()
        a, b, c = tmin > 0, tmin < 1, dmin < R2
        c1, c2, c3 = r < R2, r1 < R2, a & b & c
        d3 = torch.minimum(torch.minimum(torch.where(b & c, tmin.abs(), inf), torch.where(a & c, (tmin - 1).abs(), inf)),
                           torch.where(a & b, (dmin - R2).abs() / R2, inf))
        d3 = torch.where(w2 > 0, d3, inf)
        flag = torch.minimum(torch.minimum(torch.where(~(c2 | c3), (r - R2).abs() / R2, inf),
                                           torch.where(~(c1 | c3), (r1 - R2).abs() / R2, inf)),
                             torch.where(~(c1 | c2), d3, inf))
        m = torch.minimum(m, torch.where(pair, flag, inf).min())
    return float(m)


def step64(p, v, v0, d, prm, version, dt, radius, margins=None, dtype=torch.float64):
    """src/models/mlapm.py:10-58 in float64 under autograd on compacted agents; the discrete decisions (view, rotation
    sign, UCY collision) in float32 as the reference makes them, with the coll.unsqueeze(-1) fix.  margins: a list that
    receives this step's decision_margin.  dtype=torch.float32 (p, v, v0, d in float32): the same expressions in plain
    float32, to tell what float32 can resolve on a scene, never as a reference."""
    import torch.nn.functional as F
    prm = {k: x.to(dtype) for k, x in prm.items()}
    ed = F.normalize(d - p, dim=-1)
    if margins is not None:
        margins.append(decision_margin(p.detach(), v.detach(), ed.detach(), version, radius))
    force = (v0[:, None] * ed - v) / prm['tau']
    vr = p[None] - p[:, None]
    vv = v[None] - v[:, None]
    r = vr.norm(dim=-1)
    r = torch.where(r > 0, r, torch.zeros_like(r))
    vr32, vv32 = vr.detach().float(), vv.detach().float()
    view = (torch.einsum('nk,nmk->nm', v.detach().float(), vr32) > 0).to(dtype)
    n = F.normalize(vr, dim=-1)
    if version == 'raw':
        g = torch.exp(prm['B'] * r)
        dx, dy = n[..., 0], n[..., 1]
    else:
        cr = vr32[..., 0] * ed.detach().float()[:, None, 1] - vr32[..., 1] * ed.detach().float()[:, None, 0]
        sg = torch.where(cr > 0, -torch.ones_like(cr), torch.ones_like(cr)).to(dtype)
        th = sg * prm['theta'] / 180 * math.pi
        dx, dy = th.cos() * n[..., 0] - th.sin() * n[..., 1], th.sin() * n[..., 0] + th.cos() * n[..., 1]
        if version == 'GC':
            cs = F.cosine_similarity(vr, vv, dim=-1)
            g = torch.exp(prm['B'] * r + prm['C'] * cs + prm['D'] * r * cs)
        else:
            coll = vr32.norm(dim=-1) < radius * 2
            coll |= (vr32 + vv32 * 1.0).norm(dim=-1) < radius * 2
            tmin = -(vr32 * vv32).sum(-1) / (vv32 * vv32).sum(-1)
            dmin = ((vr32 * vr32).sum(-1) - (vr32 * vv32).sum(-1) ** 2 / (vv32 * vv32).sum(-1)).sqrt()
            coll |= (tmin > 0) & (tmin < 1) & (dmin < radius * 2)
            c = coll.to(dtype)
            g = torch.exp(prm['B'] * r * c + prm['C'] * c)
    gfac = view * prm['A'] * g
    eye = torch.eye(p.shape[0], dtype=torch.bool)
    gfac = torch.where(eye, torch.zeros_like(gfac), gfac)
    force = force - torch.stack(((gfac * dx).sum(1), (gfac * dy).sum(1)), -1)
    return v + force * dt


def _leaves(params):
    return {k: torch.tensor(float(params[k]), dtype=torch.float64, requires_grad=True) for k in NAMES}


def _grads(loss, prm, retain=False):
    if not loss.requires_grad:                                   # no term at all
        return np.zeros(len(NAMES))
    grads = torch.autograd.grad(loss, [prm[k] for k in NAMES], allow_unused=True, retain_graph=retain)
    return np.array([0.0 if x is None else float(x) for x in grads])


def fit_reference(pack, params, version, dt, radius=0.3, desired_speed=None, scale=False, dtype=torch.float64):
    """The one-step loss of a pack_clip pack in float64 under autograd: (loss, grad), with scale=True also the mean over
    the focal entries of |d loss_i / d constant| (the golden files' grad_scale).  desired_speed: float64 (N) per agent in
    place of the pack's float32 values.  No focal entry: loss 0, gradient 0.  dtype=torch.float32: every frame's step and
    residuals in plain float32, summed over the frames in float64 as the kernels sum their rows (step64)."""
    prm = _leaves(params)
    st, dst, tgt = pack.state.cpu().double(), pack.destination.cpu().double(), pack.target.cpu().double()
    v0 = pack.desired_speed.cpu().double() if desired_speed is None else \
        torch.as_tensor(desired_speed, dtype=torch.float64)[pack.agent.cpu()]
    off = pack.offsets.cpu().tolist()
    total, count, rows = torch.zeros((), dtype=torch.float64), 0, []
    for f in range(len(off) - 1):
        a, b = off[f], off[f + 1]
        fin = torch.isfinite(tgt[a:b]).all(-1)
        if not fin.any():
            continue
        pred = step64(st[a:b, :2].to(dtype), st[a:b, 2:].to(dtype), v0[a:b].to(dtype), dst[a:b].to(dtype), prm, version, dt,
                      radius, dtype=dtype)
        li = ((pred[fin] - tgt[a:b][fin].to(dtype)) ** 2).sum(-1).double()
        if scale:
            for i in range(li.shape[0]):
                g = torch.autograd.grad(li[i], [prm[k] for k in NAMES], retain_graph=True, allow_unused=True)
                rows.append([0.0 if x is None else abs(float(x)) for x in g])
        total = total + li.sum()
        count += int(fin.sum())
    if count == 0:
        return (0.0, np.zeros(6), np.zeros(6)) if scale else (0.0, np.zeros(6))
    loss = total / count
    out = float(loss.detach()), _grads(loss, prm)
    return out + (np.array(rows).mean(0),) if scale else out


def ucy_reference(pack, params, dt, radius):
    """Float64 restatement of the UCY law on a pack_clip pack: (loss, grad)."""
    return fit_reference(pack, params, 'UCY', dt, radius)


def clip_arrays(raw, desired_speed=None, skip_frames=25):
    """A clip as the rollout yardstick reads it: P, V, D (T, N, 2) float64 with 0 where absent, present (T, N) numpy bool by
    pack_clip's rule, v0 (N) float64.  desired_speed as pack_windows takes it, or float64 (N) values that are kept as
    they are."""
    from piml_amd.calibrate import _present_and_speed
    keep = torch.is_tensor(desired_speed) and desired_speed.dtype == torch.float64
    P, V, D, present, v0 = _present_and_speed(raw, None if keep else desired_speed, skip_frames)
    P, V, D = (torch.nan_to_num(x.double()) for x in (P, V, D))
    v0 = desired_speed.reshape(-1).clone() if keep else torch.nan_to_num(v0.double())
    return types.SimpleNamespace(P=P, V=V, D=D, present=present.numpy(), v0=v0)


def desired_speed64(raw, skip_frames=25):
    """data.desired_speed_per_agent's rule in float64 (N): the mean |v| over the first skip_frames frames after the agent
    starts moving, as the golden generators take it."""
    from piml_amd.calibrate import _present_and_speed
    _, V, _, present, _ = _present_and_speed(raw, None, skip_frames)
    speed = torch.where(present, V.double().norm(dim=-1), torch.zeros((), dtype=torch.float64))
    v0 = torch.zeros(speed.shape[1], dtype=torch.float64)
    for n in range(speed.shape[1]):
        mv = torch.nonzero(speed[:, n] > 0)
        if len(mv):
            v0[n] = speed[int(mv[0]):int(mv[0]) + skip_frames, n].mean()
    return v0


def perturbed(clip, rel, seed):
    """clip_arrays' result with every recorded velocity moved by a relative N(0, rel) (the floor of a long rollout)."""
    g = torch.Generator().manual_seed(seed)
    out = copy.copy(clip)
    out.V = clip.V * (1.0 + rel * torch.randn(clip.V.shape, generator=g, dtype=torch.float64))
    return out


def _window_terms(c, t0, H, prm, version, dt, radius, decay, sse, cnt, margins=None):
    """(weighted numerator, weight) of the window t0 .. t0 + H of one clip; adds its per-step sums to sse and cnt."""
    p, v = c.P[t0].clone(), c.V[t0].clone()
    num, wsum = torch.zeros((), dtype=torch.float64), 0.0
    for k in range(H):
        t = t0 + k
        idx = torch.tensor(np.nonzero(c.present[t])[0], dtype=torch.long)
        vn = step64(p[idx], v[idx], c.v0[idx], c.D[t, idx], prm, version, dt, radius, margins)
        car = torch.tensor(c.present[t] & c.present[t + 1])
        vfull = torch.zeros_like(p).index_copy(0, idx, vn)
        pfull = torch.zeros_like(p).index_copy(0, idx, p[idx] + vn * dt)
        p = torch.where(car[:, None], pfull, c.P[t + 1])
        v = torch.where(car[:, None], vfull, c.V[t + 1])
        e2 = ((p[car] - c.P[t + 1][car]) ** 2).sum(-1)
        w = decay ** (H - k - 1)                                  # 0 ** 0 = 1: decay 0 keeps k = H alone
        num = num + w * e2.sum()
        wsum += w * int(car.sum())
        sse[k] += float(e2.detach().sum())
        cnt[k] += int(car.sum())
    return num, wsum


def rollout_reference(raw, starts, H, params, version, dt, radius=0.3, decay=1.0, desired_speed=None, clips=None,
                      scale=False):
    """The windowed rollout loss of pack_windows' windows in float64 under autograd: (loss, grad, per-step sse, counts),
    with scale=True also sum over the windows of |d numerator_w / d constant| / sum w (the golden file's grad_scale).
    raw: a RawData or a clip_arrays result, or a list of them with clips[w] the clip of window w (pack.clip) and
    desired_speed one value per clip.  No term at all: loss 0, gradient 0."""
    many = isinstance(raw, (list, tuple))
    raws = list(raw) if many else [raw]
    speeds = list(desired_speed) if many and isinstance(desired_speed, (list, tuple)) else [desired_speed] * len(raws)
    arr = [r if hasattr(r, 'present') else clip_arrays(r, s) for r, s in zip(raws, speeds)]
    clips = [0] * len(starts) if clips is None else clips
    prm = _leaves(params)
    num, wsum, sse, cnt, rows = torch.zeros((), dtype=torch.float64), 0.0, np.zeros(H), np.zeros(H), []
    for c, t0 in zip(clips, starts):
        n_w, w_w = _window_terms(arr[c], int(t0), H, prm, version, dt, radius, decay, sse, cnt)
        if scale:
            rows.append(np.abs(_grads(n_w, prm, retain=True)))
        num, wsum = num + n_w, wsum + w_w
    if wsum == 0:
        out = 0.0, np.zeros(6), sse, cnt
        return out + (np.zeros(6),) if scale else out
    loss = num / wsum
    out = float(loss.detach()), _grads(loss, prm), sse, cnt
    return out + (np.array(rows).sum(0) / wsum,) if scale else out


def rollout_margin(raw, starts, H, params, version, dt, radius=0.3, desired_speed=None, clips=None):
    """The smallest decision_margin over every step of the float64 rollouts of rollout_reference's windows.  A float32
    rollout takes a decision whose margin is within its own rounding either way, and one pair's term with it."""
    many = isinstance(raw, (list, tuple))
    raws = list(raw) if many else [raw]
    speeds = list(desired_speed) if many and isinstance(desired_speed, (list, tuple)) else [desired_speed] * len(raws)
    arr = [r if hasattr(r, 'present') else clip_arrays(r, s) for r, s in zip(raws, speeds)]
    prm = {k: torch.tensor(float(params[k]), dtype=torch.float64) for k in NAMES}
    margins = []
    with torch.no_grad():
        for c, t0 in zip([0] * len(starts) if clips is None else clips, starts):
            _window_terms(arr[c], int(t0), H, prm, version, dt, radius, 1.0, np.zeros(H), np.zeros(H), margins)
    return min(margins) if margins else float('inf')


def grad_scale(gw):
    """check_against's scale of each gradient: its own magnitude and a thousandth of the largest one's."""
    return np.maximum(np.abs(gw), 1e-3 * np.abs(gw).max())


def worst_error(loss, grad, want, gw):
    """The largest of the loss's relative error and the gradients' errors on check_against's scale (0 for 0 against 0)."""
    el = abs(loss - want) / want if want else abs(loss)
    s = grad_scale(gw)
    eg = np.where(s > 0, np.abs(grad - gw) / np.where(s > 0, s, 1.0), np.abs(grad))
    return max(el, float(eg.max()))


def check_against(loss, grad, ps, want, gw, sse, cnt, rel=1e-5, version=None):
    """The bars of every comparison with the yardstick.  ps / sse / cnt None: no per-step columns (the one-step fit).
    version: the constants it does not use must then be exactly 0."""
    assert abs(loss - want) <= rel * want, (loss, want)
    # each gradient against its own magnitude and the largest one's (a sum with cancellations)
    bar = rel * np.maximum(np.abs(gw), 1e-3 * np.abs(gw).max())
    assert (np.abs(grad - gw) <= bar + rel * np.abs(gw)).all(), (grad, gw)
    if version is not None:
        for q in UNUSED[version]:
            assert grad[q] == 0.0 and gw[q] == 0.0, (version, NAMES[q], grad[q], gw[q])
    if ps is None:
        return
    H = len(sse)
    assert np.array_equal(ps[H:], cnt)
    assert np.allclose(ps[:H], sse, rtol=10 * rel, atol=0), (ps[:H], sse)


# ---- scenes -------------------------------------------------------------------------------------------------------------
def flow_clip(N, T, law, version='GC', spacing=1.5, jitter=0.15, heading_deg=27, seed=0, dt=0.08, speed=1.3, radius=0.3):
    """A RawData of T frames: N agents start on a jittered square lattice (`spacing` apart, each coordinate moved by up to
    `jitter` of it), all heading the same way, `heading_deg` off the lattice axes so that no near neighbour sits abeam
    (where the view test would hang on a rounding), towards destinations 200 m ahead.  Simulated in float64 by step64 at
    the law `law`, stored as float32; every agent's desired speed is `speed`."""
    from piml_amd.data.data import RawData
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil(math.sqrt(N)))
    ij = torch.stack(torch.meshgrid(torch.arange(side), torch.arange(side), indexing='ij'), -1).reshape(-1, 2)[:N]
    p = (ij.double() + jitter * (2 * torch.rand(N, 2, generator=g, dtype=torch.float64) - 1)) * spacing
    a = math.radians(heading_deg)
    head = torch.tensor([math.cos(a), math.sin(a)], dtype=torch.float64)
    v = speed * head * (0.8 + 0.4 * torch.rand(N, 1, generator=g, dtype=torch.float64)) \
        + 0.1 * torch.randn(N, 2, generator=g, dtype=torch.float64)
    d = p + 200.0 * head
    v0 = torch.full((N,), float(speed), dtype=torch.float64)
    prm = {k: torch.tensor(float(law[k]), dtype=torch.float64) for k in NAMES}
    P, V = [p], [v]
    with torch.no_grad():
        for _ in range(T - 1):
            v = step64(p, v, v0, d, prm, version, dt, radius)
            p = p + v * dt
            P.append(p)
            V.append(v)
    return RawData(position=torch.stack(P).float(), velocity=torch.stack(V).float(),
                   destination=d.float().expand(T, N, 2).clone(), meta_data={'time_unit': dt})


def with_presence(raw, edits):
    """A copy of the clip with NaN spans: edits = {agent: [(first, stop), ...]} makes the agent absent in frames
    first .. stop - 1 (position and velocity NaN, which is pack_clip's presence rule)."""
    from piml_amd.data.data import RawData
    P, V = raw.position.clone(), raw.velocity.clone()
    for agent, spans in edits.items():
        for a, b in spans:
            P[a:b, agent] = float('nan')
            V[a:b, agent] = float('nan')
    return RawData(position=P, velocity=V, destination=raw.destination.clone(), meta_data={'time_unit': raw.time_unit})


def presence_patterns(t0, H, T, k=3, gap=2):
    """The NaN spans (with_presence) that give a slot of the window t0 .. t0 + H of a T-frame clip each pattern the flag
    byte encodes, by name.  1 <= k, k + gap <= H - 1."""
    return {'leave': [(t0 + k, T)],                               # present in 0 .. k - 1
            'enter': [(0, t0 + k)],                               # injected in k
            'gap': [(t0 + k, t0 + k + gap)],                      # leaves in k, injected again in k + gap
            'first_only': [(t0 + 1, T)],                          # frame 0 alone: a source of step 0, no term
            'last_only': [(0, t0 + H)],                           # frame H alone: injected where nothing follows
            'one_mid': [(0, t0 + k), (t0 + k + 1, T)]}            # one mid-window frame: a source of step k, no term


def expected_flags(name, H, k=3, gap=2):
    """The H + 1 flag bytes of a slot with presence_patterns' pattern `name`, written out by hand."""
    first, kept = PRESENT | INJECTED, PRESENT | CARRIED
    return {'leave': [first] + [kept] * (k - 1) + [0] * (H + 1 - k),
            'enter': [0] * k + [first] + [kept] * (H - k),
            'gap': [first] + [kept] * (k - 1) + [0] * gap + [first] + [kept] * (H - k - gap),
            'first_only': [first] + [0] * H,
            'last_only': [0] * H + [first],
            'one_mid': [0] * k + [first] + [0] * (H - k)}[name]


def frames_of_sizes(sizes, law, version='GC', seed=0, finite_targets=None, **kw):
    """(raw, target) for pack_clip: frame f of the clip holds sizes[f] agents, a seeded random subset of a flow_clip of
    max(sizes) agents, and every present entry's target is its velocity in the next frame of the full simulation.
    finite_targets = {frame: m} keeps the targets of the frame's first m present agents and makes the others NaN: those
    entries are still sources and no longer focal."""
    F, N = len(sizes), max(sizes)
    full = flow_clip(N, F + 1, law, version, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    edits, target = {}, full.velocity[1:].clone()
    target = torch.cat((target, torch.full((1, N, 2), float('nan'))), 0)
    for f, n in enumerate(sizes):
        order = torch.randperm(N, generator=g).tolist()
        for a in order[n:]:
            edits.setdefault(a, []).append((f, f + 1))
        m = (finite_targets or {}).get(f)
        if m is not None:
            for a in sorted(order[:n])[m:]:
                target[f, a] = float('nan')
    return with_presence(full, edits), target


# ---- pack editors -------------------------------------------------------------------------------------------------------
def _copy(pack):
    return types.SimpleNamespace(**{k: v for k, v in vars(pack).items() if k != 'workspace'})


def with_windows(pack, small, big):
    """The pack_windows pack with the window lists `small` and `big` (window indices): big_base and big_slots rebuilt.
    The kernels run whatever list names a window; only the small form needs n <= 64 and horizon <= 48."""
    out = _copy(pack)
    dev = pack.small_windows.device
    cnt = [pack.slot_count[w] for w in big]
    assert all(pack.slot_count[w] <= 64 for w in small) and (not small or pack.horizon <= 48)
    out.small_windows = torch.tensor(sorted(small), dtype=torch.int32, device=dev)
    out.big_windows = torch.tensor(list(big), dtype=torch.int32, device=dev)
    out.big_base = torch.tensor([sum(cnt[:i]) for i in range(len(cnt))], dtype=torch.int32, device=dev)
    out.big_slots = int(sum(cnt))
    return out


def as_big(pack):
    """Every window in the big form."""
    return with_windows(pack, [], sorted(pack.small_windows.tolist() + pack.big_windows.tolist()))


def only_small(pack):
    return with_windows(pack, pack.small_windows.tolist(), [])


def only_big(pack):
    return with_windows(pack, [], pack.big_windows.tolist())


def as_wave(pack):
    """Every focal entry of a pack_clip pack in the wave form (the kernels loop over whatever frame the entry names)."""
    out = _copy(pack)
    out.big_focal = torch.sort(torch.cat((pack.small_focal, pack.big_focal))).values.contiguous()
    out.small_focal = pack.small_focal[:0].clone()
    return out


def as_lane(pack):
    """Every focal entry of a pack_clip pack in the lane form."""
    out = _copy(pack)
    out.small_focal = torch.sort(torch.cat((pack.small_focal, pack.big_focal))).values.contiguous()
    out.big_focal = pack.big_focal[:0].clone()
    return out
