"""A float64 restatement of one window of the fine-tuning rollout (HOT LOOP C) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain torch, CPU or GPU, differentiable by autograd, nothing of piml_amd in its arithmetic: the frame step
(src/models/simulators.py:741-769), the relative features by GATHERS through imposed neighbour indices (include/piml_hip.h:79-83;
selection is discrete, so the indices come from the float32 run under test), the model's tail under the agent-axis norm
(quirk Q2), a stand-in model of two fixed linear maps between the frames, and the rollout losses (the header of
piml_amd/csrc/losses.hip).  tests/test_rollout_window_ref.py pins it; tests/test_rollout_window_gpu.py measures the HIP frame
node against it.  `make_case` builds the seeded scenes both files use.
"""
import numpy as np
import torch

DT = 0.08
TAU = 2.0
THR = 1.5            # collision threshold of the count records (large enough that the synthetic crowds do collide)
DECAY = 0.9
W_COLL, W_HARD = 0.7, 2.1
KINDS = ('apred', 'sum', 'sum_obs', 'ksum')


def nan0(x):
    """NaN -> 0 with the gradient cut on the zeroed components."""
    return torch.where(x.isnan(), torch.zeros_like(x), x)


def gather_waypoints(waypoints, idx):
    """waypoints (D, N, 2) or (C, D, N, 2), idx (C, N) -> (C, N, 2)"""
    C, N = idx.shape
    n = torch.arange(N, device=idx.device).expand(C, N)
    if waypoints.dim() == 3:
        return waypoints[idx, n]
    c = torch.arange(C, device=idx.device).unsqueeze(1).expand(C, N)
    return waypoints[c, idx, n]


def frame_step(p, v, a, a_next, dest, dest_idx, waypoints, dest_num, dt, new=None, truth=None):
    """One frame between the model call and the features: lagged Euler, waypoint switch at < 0.5 m, idx -= idx > dest_num - 1,
    gather of the next waypoint, injection of `truth` = (p, v, a, dest, dest_idx) of the next frame where `new` (C, N) bool is
    set, NaN -> 0 on the new velocity and acceleration.  -> (p', v', a', dest', dest_idx', |p - dest| (C, N))."""
    v_next = v + a * dt
    p_next = p + v * dt
    d = (p - dest).detach()
    dist = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    idx = dest_idx + (dist < 0.5).long()
    idx = idx - (idx > dest_num - 1).long()
    dest_next = gather_waypoints(waypoints, idx)
    a_new = a_next
    if new is not None:
        m = new.unsqueeze(-1)
        p_next = torch.where(m, truth[0], p_next)
        v_next = torch.where(m, truth[1], v_next)
        a_new = torch.where(m, truth[2], a_new)
        dest_next = torch.where(m, truth[3], dest_next)
        idx = torch.where(new, truth[4], idx)
    return p_next, nan0(v_next), nan0(a_new), dest_next, idx, dist


def gathered_features(p, v, a, dest, obstacles, speed, ped_idx, obs_idx):
    """ped (C, N, kp, 6) = (p_j - p_i, v_j - v_i, a_j - a_i), obs (C, N, ko, 6) = (o_j - p_i, -v_i, -a_i), empty slots (index -1)
    zero, self (C, N, 7) = [dest - p (NaN -> 0), v, a, v0]; NaN velocities / accelerations read as 0."""
    C, N = p.shape[0], p.shape[1]
    v, a = nan0(v), nan0(a)
    state = torch.cat((p, v, a), dim=-1)
    me = state.unsqueeze(2)
    c = torch.arange(C, device=p.device).view(C, 1, 1)
    ped_idx, obs_idx = ped_idx.long(), obs_idx.long()
    pf = torch.where((ped_idx >= 0).unsqueeze(-1), state[c, ped_idx.clamp_min(0)] - me, torch.zeros((), dtype=p.dtype, device=p.device))
    if obs_idx.shape[-1]:
        o = torch.cat((obstacles.reshape(-1, 2), torch.zeros(obstacles.reshape(-1, 2).shape[0], 4, dtype=p.dtype, device=p.device)), dim=-1)
        of = torch.where((obs_idx >= 0).unsqueeze(-1), o[obs_idx.clamp_min(0)] - me, torch.zeros((), dtype=p.dtype, device=p.device))
    else:
        of = torch.zeros(C, N, 0, 6, dtype=p.dtype, device=p.device)
    sf = torch.cat((nan0(dest - p), v, a, speed.reshape(C, N, 1)), dim=-1)
    return pf, of, sf


def agent_norm_tail(acc_ped, acc_obs, sf, tau):
    """sum_k acc_ped (+ sum_k acc_obs) + (v0 d / t - v) / tau with t the norm of d's component over the AGENTS of the slice,
    0 -> 0.1 (quirk Q2).  acc (C, N, 2) or (C, N, k, 2)."""
    s = acc_ped.sum(dim=2) if acc_ped.dim() == 4 else acc_ped
    if acc_obs is not None:
        s = s + (acc_obs.sum(dim=2) if acc_obs.dim() == 4 else acc_obs)
    d = sf[..., 0:2]
    sq = (d * d).sum(dim=1, keepdim=True)                                  # (C, 1, 2)
    zero = sq == 0
    t = torch.where(zero, torch.full_like(sq, 0.1), torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)))
    return s + (sf[..., 6:7] * (d / t) - sf[..., 2:4]) / tau


def standin_model(pf, of, sf, Wp, Wo, kind, tau):
    """The stand-in model: acc_ped = pf @ Wp per neighbour row, acc_obs = of @ Wo, sf passes through -> the prediction."""
    acc_p, acc_o = pf @ Wp, (of @ Wo if kind != 'sum' else None)
    return agent_norm_tail(acc_p, acc_o, sf, tau)


def window_losses(p_res, labels, mask_pred, gates, records, abn, decay, w_coll, w_hard):
    """The rollout losses on the stacked positions (C, T, N, 2); records: per frame None or (2, C, N) collision counts.
    -> (total, mse, w_coll * focus, w_hard * hard focus, stats (3,))"""
    C, T, N = p_res.shape[:3]
    keep = (mask_pred != 0).unsqueeze(-1)
    gate4 = gates.view(1, T, 1, 1)
    p = torch.where(keep & gate4, p_res, torch.zeros_like(p_res))
    lab = torch.where(keep, labels[..., :2].to(p.dtype), torch.zeros_like(p_res))
    w = torch.pow(torch.tensor(float(decay), dtype=p.dtype, device=p.device),
                  (T - 1 - torch.arange(T, device=p.device)).to(p.dtype)).view(1, T, 1, 1)
    mse = ((p - lab) ** 2 * w).sum()
    n = lab[:, T - 1] - lab[:, 0]
    n = (n / (torch.sqrt((n * n).sum(-1, keepdim=True)) + 1e-6)).unsqueeze(1)
    perp = lambda x: x - (x * n).sum(-1, keepdim=True) * n
    avoid = (perp(p) - perp(lab)) ** 2 * w
    z = torch.zeros(2, C, N, dtype=p.dtype, device=p.device)
    rec = torch.stack([z if r is None else r.to(p.dtype) for r in records], dim=2) * gates.to(p.dtype).view(1, 1, T, 1)  # (2, C, T, N)
    am = abn.to(p.dtype).view(1, 1, N, 1)
    focus = [(((rec[q].sum(dim=1) > 0).to(p.dtype)).view(C, 1, N, 1) * avoid * am).sum() for q in (0, 1)]
    stats = torch.stack((rec[0].sum(), rec[1].sum(), (mask_pred == 1).sum().to(p.dtype)))
    return mse + w_coll * focus[0] + w_hard * focus[1], mse, w_coll * focus[0], w_hard * focus[1], stats


def window(case, p, v, a, feats0, Wp, Wo, kind, t_start, select, dt=DT, tau=TAU):
    """The frames t_start .. T - 1 of `case` (tensors of one dtype / device, see make_case / case_to) from the state (p, v, a) and
    the initial features feats0 = (pf, of, sf).  select(t, p', v', a', dest') -> (ped_idx, obs_idx) of the new state.
    -> dict(inputs = the position every frame starts from, frames = per frame (p', v', a', dest', idx', pf, of, sf),
    sf_in = the self features every frame's model call read, margin = per frame | |p - dest| - 0.5 | over present agents,
    near = per frame the number of agents inside the radius)"""
    T = case['position'].shape[1]
    dest, idx = case['destination'][:, t_start], case['dest_idx'][:, t_start]
    new_flag = (case['mask_p'] - case['mask_p_pred']).long() == 1
    speed = case['self_features'][:, t_start, :, 6:]
    state = feats0
    out = dict(inputs=[], frames=[], sf_in=[], margin=[], near=[])
    for t in range(t_start, T):
        out['sf_in'].append(state[2])
        a_next = standin_model(*state, Wp, Wo, kind, tau)
        out['inputs'].append(p)
        new = truth = None
        if t + 1 < T:
            new = new_flag[:, t + 1]
            truth = tuple(case[k][:, t + 1] for k in ('position', 'velocity', 'acceleration', 'destination', 'dest_idx'))
        p, v, a, dest, idx, dist = frame_step(p, v, a, a_next, dest, idx, case['waypoints'], case['dest_num'], dt, new, truth)
        out['margin'].append((dist - 0.5).abs()[~dist.isnan()])
        out['near'].append(int((dist < 0.5).sum()))
        pi, oi = select(t, p.detach(), v.detach(), a.detach(), dest)
        state = gathered_features(p, v, a, dest, case['obstacles'], speed, pi, oi)
        out['frames'].append((p, v, a, dest, idx, *state))
    return out


def make_case(C, T, N, M, seed, wp_per_slice=False, closed_gate=True):
    """A seeded window (CPU, float32 / int64): series (C, T, N, .) with ~10 % of the agents absent (NaN) until a later frame,
    masks that re-initialise ~20 % of the present agents per frame from the series, one frame nobody is predicted in, a NaN in
    an injected velocity and in an injected acceleration, waypoints some agents stand next to, labels, count-loss mask."""
    from piml_amd.scenes import synthetic_gc_scene
    rng = np.random.default_rng(seed)
    sc = synthetic_gc_scene(N, max(M, 1), seed=seed, nan_frac=0.0, channels=C)
    p0, v0, dest0, speed = sc['position'], sc['velocity'], sc['destination'], sc['desired_speed']
    t_ax = np.arange(T, dtype=np.float32).reshape(1, T, 1, 1)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    pos = p0[:, None] + v0[:, None] * (DT * t_ax) + 0.05 * f32(C, T, N, 2)
    vel = v0[:, None] + 0.1 * f32(C, T, N, 2)
    acc = 0.3 * f32(C, T, N, 2)
    D = 4
    dest_num = rng.integers(1, D + 1, size=N)
    dest_idx = (rng.integers(0, D, size=(C, T, N)) % dest_num).astype(np.int64)
    way = (rng.random((C, D, N, 2)) * 30).astype(np.float32)
    if not wp_per_slice:
        way = np.broadcast_to(way[:1], way.shape).copy()
    # the destination of frame t is the waypoint its index names; ~15 % of the agents stand 0.2 m from it (channel 0 when shared)
    cc, nn = np.meshgrid(np.arange(C), np.arange(N), indexing='ij')
    close = rng.random((C, N)) < 0.15
    ang = rng.random((C, N)) * 6.28
    spot = p0 + 0.2 * np.stack((np.cos(ang), np.sin(ang)), -1).astype(np.float32)
    for c in range(C if wp_per_slice else 1):
        sel = close[c]
        way[c if wp_per_slice else slice(None), dest_idx[c, 0][sel], np.arange(N)[sel]] = spot[c][sel]
    dest = way[cc[:, None], dest_idx, nn[:, None]]                                   # (C, T, N, 2)
    # presence: entry frame 0 (there from the start), 1 .. T - 1 (absent before) or T (never)
    entry = np.where(rng.random((C, N)) < 0.1, rng.integers(1, T + 1, size=(C, N)), 0)
    if N == 1:
        entry[:] = 0
    tt = np.arange(T).reshape(1, T, 1)
    mask_p = (tt >= entry[:, None]).astype(np.float32)
    mask_pred = mask_p * (rng.random((C, T, N)) > 0.2) * (tt != entry[:, None])
    mask_pred[:, 0] = mask_p[:, 0] * (rng.random((C, N)) > 0.2)
    if T > 2 and closed_gate:
        mask_pred[:, T - 2] = 0                                                       # a frame nobody is predicted in
    mask_pred = mask_pred.astype(np.float32)
    absent = mask_p == 0
    pos[absent], dest[absent] = np.nan, np.nan          # as the data sets mark them: position and destination NaN,
    vel[absent], acc[absent] = 0.0, 0.0                  # velocity and acceleration zero
    new = (mask_p - mask_pred) == 1
    new[:, 0] = False
    hits = np.argwhere(new)
    hits = hits[hits[:, 1] >= min(2, T - 1)]          # (behind every t_start the tests use: the initial state stays free of them)
    if len(hits) >= 2:
        c, t, n = hits[len(hits) // 3]
        vel[c, t, n, 0] = np.nan                                                      # the zero_mask gradient cut
        c, t, n = hits[2 * len(hits) // 3]
        acc[c, t, n, 1] = np.nan
    labels = np.concatenate((pos + 0.3 * f32(C, T, N, 2), f32(C, T, N, 5)), -1)
    labels[absent] = np.nan
    sf = f32(C, T, N, 7)
    sf[..., 6] = speed.reshape(C, 1, N)
    obstacles = sc['obstacles'] if M > 0 else np.zeros((0, 2), np.float32)
    tens = dict(position=pos, velocity=vel, acceleration=acc, destination=dest, dest_idx=dest_idx, waypoints=way if wp_per_slice else way[0],
                dest_num=dest_num.astype(np.int64), mask_p=mask_p, mask_p_pred=mask_pred, labels=labels, self_features=sf,
                obstacles=obstacles, abnormal=(rng.random(N) > 0.1).astype(np.float32))
    case = {k: torch.from_numpy(np.ascontiguousarray(x)) for k, x in tens.items()}
    g = torch.Generator().manual_seed(seed)
    case['Wp'] = torch.randn(6, 2, generator=g) * 0.2
    case['Wo'] = torch.randn(6, 2, generator=g) * 0.2
    return case


def case_to(case, device, dtype):
    return {k: (x.to(device=device, dtype=dtype) if x.is_floating_point() else x.to(device)) for k, x in case.items()}


def oracle_select(case32, topk=(6, 10)):
    """select() for the CPU: the indices the float32 oracle picks on the float32 image of the state."""
    from oracle import oracle
    obstacles = case32['obstacles'].numpy()

    def select(t, p, v, a, dest):
        if obstacles.shape[0] == 0:
            far = np.array([[1e4, 1e4]], np.float32)
            r = oracle.relfeat_fwd(*[x.float().numpy()[:, None] for x in (p, v, a, dest)], far, return_index=True)
            return torch.from_numpy(r[3][:, 0].astype(np.int64)), torch.zeros(*p.shape[:2], 0, dtype=torch.int64)
        r = oracle.relfeat_fwd(*[x.float().numpy()[:, None] for x in (p, v, a, dest)], obstacles, return_index=True)
        return torch.from_numpy(r[3][:, 0].astype(np.int64)), torch.from_numpy(r[4][:, 0].astype(np.int64))
    return select


# the cases of tests/test_rollout_window_gpu.py: (C, T, N, M, seed, waypoints per slice, a closed gate at frame T - 2).  A closed
# gate re-initialises every agent, which cuts every gradient chain through that frame: n300 goes without, so that the rollout
# loss alone reaches the model calls of frames 0 and 1 through the features.
SHAPES = {'one': (1, 2, 1, 0, 11, False, False), 'odd63': (3, 4, 63, 3, 12, False, True), 'n257': (2, 4, 257, 40, 13, True, True),
          'n300': (3, 5, 300, 40, 14, True, False)}
