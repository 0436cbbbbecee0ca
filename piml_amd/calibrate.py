"""Calibrate MLAPM's constants (tau, A, B, C, D, theta) to a clip on the GPU.

    python -m piml_amd.calibrate --data clip.npy [clip2.npy ...] --version GC [--init A=7.55,B=-3] [--fit A,B,theta]
                                 [--frames a:b] [--valid_frames c:d] [--horizon H [--stride S] [--time_decay g]]
                                 [--steps N] --out params.json

The clip is a recorded GC / UCY clip, or one that `python -m piml_amd.simulate` wrote with a trained PINNSF: fitting the
closed-form law to the network's own trajectories distils it into MLAPM's six constants.  The loss is the mean squared
residual of one MLAPM.step per (frame, agent) against the agent's velocity in the next frame, and its gradient with
respect to the constants is analytic (piml_mlapm_fit_loss_grad, one pass over the pairs).  With --horizon H the loss is
instead the mean squared position error of H closed-loop MLAPM steps per window, the law's own errors fed back through
the neighbours as `simulate --law mlapm` runs it (piml_mlapm_rollout_fit_loss_grad, forward and adjoint in one launch).
`MLAPM(**result.params)` simulates with the result.

    python -m piml_amd.calibrate --data clip.npy --version UCY --match-stats [--match crowd,pairs] [--scene-frames a:b]
                                 [--scene-jitter x] [--seeds 0:8] [--population 16] [--generations 30] [--search-seed 0]
                                 [--init ...] [--fit A,B] --out params.json

--match-stats fits the law to crowd statistics instead of trajectories (calibrate_mlapm_to_stats): the clip becomes an
open-world scene (scenarios.clip_scenario), every generation of a derivative-free search runs population x seeds members
in one ensemble (MLAPM.simulate_sweep's law table), and the objective is the distance between each candidate's pooled
crowd / pair statistics and the clip's own (stats_objective).

    python -m piml_amd.calibrate --data clip.npy --match-stats --scene-groups auto|FILE.json --fit Ag,group_dist --init Ag=3
                                 [--match crowd,pairs,groups] --out grouped.json

--scene-groups keeps the clip's groups as arrival units (scenarios.clip_scenario(groups=)), the candidates run the group
cohesion term (Ag, group_dist) and the group statistics join the objective; grouped.json is what
`simulate --params` reads."""
import argparse
import json
import math
import os
import sys
import types

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')      # before torch brings the HIP runtime up (piml_amd.hip_graphs_safe)

import torch  # noqa: E402

PARAM_NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
# the wall term of the scene runs (MLAPM(..., Aw=, Bw=)): fitted by calibrate_mlapm_to_stats only, and never by default
WALL_PARAM_NAMES = ('Aw', 'Bw')
# the group term of a grouped clip scene's runs (MLAPM(..., Ag=[, group_dist=])): fitted by calibrate_mlapm_to_stats only
GROUP_PARAM_NAMES = ('Ag', 'group_dist')
NOISE_PARAM_NAMES = ('An', 'noise_tau')       # the fluctuation term of the scene runs: fitted by calibrate_mlapm_to_stats only
# the constants src/main_mlapm.py:16 types in
DEFAULT_INIT = {'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
SMALL_FRAME = 64          # frames up to this many agents: a lane per focal agent; above: a wave per focal agent


def _frame_list(frames, T):
    if frames is None:
        return list(range(T))
    if isinstance(frames, slice):
        return list(range(T))[frames]
    if isinstance(frames, str):
        a, b = frames.split(':')
        return list(range(T))[slice(int(a) if a else None, int(b) if b else None)]
    return [int(f) for f in frames]


def pack_clip(raw_data, frames=None, desired_speed=None, skip_frames=25, target=None, device=None):
    """A clip as the fit kernel reads it, built once per fit.

    raw_data: a `RawData` (loaded clip, or `ScenarioResult.to_raw_data()`), or a list of them: the frames of a fit are
    independent, so several clips pack as the concatenation of their single packs (frames, entries and focal lists in
    clip order; `desired_speed` / `target` then a list with one value per clip, or one scalar speed for all; every clip's
    time unit must agree).  An agent is present in frame t when its
    position, velocity and destination are finite there and (where the clip has `mask_v`) its velocity is not the
    loader's placeholder of its last frame.  Present agents are compacted frame-major (CSR): `offsets` (F + 1) int32,
    then per entry `state` (p, v), `destination`, `desired_speed`, `target`; the entries of a frame are its only sources.
    frames: which frames of the clip (None = all; a slice, 'a:b' or a list of frame indices).
    desired_speed: (N) / (N, 1) / scalar per agent; default the mean |v| over the first `skip_frames` frames after the
    agent starts moving (`data.desired_speed_per_agent`, the rule of TimeIndexedPedData.make_dataset).
    target: (T, N, 2) velocities to fit (e.g. a model's predictions); default v of frame t + 1 where the agent is present
    then, NaN (no loss term) otherwise.  Entries with a finite target are the focal entries."""
    from .data.data import desired_speed_per_agent
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    if isinstance(raw_data, (list, tuple)):
        return _pack_clips(raw_data, frames, desired_speed, skip_frames, target, device)
    P = torch.as_tensor(raw_data.position).detach().float().cpu()
    V = torch.as_tensor(raw_data.velocity).detach().float().cpu()
    D = torch.as_tensor(raw_data.destination).detach().float().cpu()
    T, N = P.shape[0], P.shape[1]
    present = torch.isfinite(P).all(-1) & torch.isfinite(V).all(-1) & torch.isfinite(D).all(-1)
    mask_v = getattr(raw_data, 'mask_v', None)
    if mask_v is not None:
        present &= torch.as_tensor(mask_v).cpu() != 0
    if target is None:
        tgt = torch.full((T, N, 2), float('nan'))
        if T > 1:
            tgt[:-1] = torch.where(present[1:].unsqueeze(-1), V[1:], tgt[1:])
    else:
        tgt = torch.as_tensor(target).detach().float().cpu()
        if tuple(tgt.shape) != (T, N, 2):
            raise ValueError(f'target must be (T, N, 2) = {(T, N, 2)}, got {tuple(tgt.shape)}')
    if desired_speed is None:
        v0 = desired_speed_per_agent(torch.where(present.unsqueeze(-1), V, torch.zeros_like(V)), skip_frames)
    else:
        v0 = torch.as_tensor(desired_speed, dtype=torch.float32).detach().cpu().reshape(-1)
        v0 = v0.expand(N).clone() if v0.numel() == 1 else v0
        if v0.numel() != N:
            raise ValueError(f'desired_speed must hold N={N} values, got {v0.numel()}')
    fl = _frame_list(frames, T)
    fr = torch.tensor(fl, dtype=torch.long)
    sub = present[fr] if len(fl) else torch.zeros(0, N, dtype=torch.bool)
    f_idx, agent = sub.nonzero(as_tuple=True)                             # frame-major, agents ascending
    t_idx = fr[f_idx] if len(fl) else f_idx
    counts = sub.sum(1)
    offsets = torch.zeros(len(fl) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    E = int(offsets[-1])
    if E >= 2 ** 31:
        raise ValueError(f'{E} entries: more than the kernel indexes (int32)')
    state = torch.cat((P[t_idx, agent], V[t_idx, agent]), -1)
    target_e = tgt[t_idx, agent]
    focal = torch.isfinite(target_e).all(-1)
    small = (counts[f_idx] <= SMALL_FRAME)
    e_idx = torch.arange(E, dtype=torch.int32)
    i32 = lambda x: x.to(torch.int32).contiguous().to(device)                 # noqa: E731
    f32 = lambda x: x.to(torch.float32).contiguous().to(device)               # noqa: E731
    return types.SimpleNamespace(
        state=f32(state), destination=f32(D[t_idx, agent]), desired_speed=f32(v0[agent]), target=f32(target_e),
        offsets=i32(offsets), frame_of=i32(f_idx), small_focal=i32(e_idx[focal & small]), big_focal=i32(e_idx[focal & ~small]),
        frames=fl, frame=t_idx, agent=agent, num_entries=E, num_focal=int(focal.sum()),
        time_unit=float(getattr(raw_data, 'time_unit', 0.0) or 0.0))


def _clip_time_unit(clips):
    units = [float(getattr(c, 'time_unit', 0.0) or 0.0) for c in clips]
    if any(not math.isclose(u, units[0], rel_tol=1e-9, abs_tol=0.0) for u in units):
        raise ValueError(f'the clips have different time units: {units}')
    return units[0]


def _per_clip(value, clips, name):
    if isinstance(value, (list, tuple)):
        if len(value) != len(clips):
            raise ValueError(f'{name}: one value per clip ({len(clips)}), got {len(value)}')
        return list(value)
    if value is not None and name == 'target':
        raise ValueError('target: one (T, N, 2) tensor per clip')
    return [value] * len(clips)


def _pack_clips(clips, frames, desired_speed, skip_frames, target, device):
    """pack_clip of several clips: the concatenation of their single packs."""
    if not clips:
        raise ValueError('no clip to pack')
    unit = _clip_time_unit(clips)
    packs = [pack_clip(c, frames=frames, desired_speed=ds, skip_frames=skip_frames, target=tg, device=device)
             for c, ds, tg in zip(clips, _per_clip(desired_speed, clips, 'desired_speed'), _per_clip(target, clips, 'target'))]
    e0 = [0]
    f0 = [0]
    for p in packs:
        e0.append(e0[-1] + p.num_entries)
        f0.append(f0[-1] + len(p.frames))
    if e0[-1] >= 2 ** 31:
        raise ValueError(f'{e0[-1]} entries: more than the kernel indexes (int32)')
    cat = lambda name: torch.cat([getattr(p, name) for p in packs])            # noqa: E731
    shifted = lambda name, base: torch.cat([getattr(p, name) + b for p, b in zip(packs, base)])  # noqa: E731
    offsets = torch.cat([packs[0].offsets[:1]] + [p.offsets[1:] + e for p, e in zip(packs, e0)])
    return types.SimpleNamespace(
        state=cat('state'), destination=cat('destination'), desired_speed=cat('desired_speed'), target=cat('target'),
        offsets=offsets, frame_of=shifted('frame_of', f0), small_focal=shifted('small_focal', e0),
        big_focal=shifted('big_focal', e0), frames=[f for p in packs for f in p.frames], frame=cat('frame'),
        agent=cat('agent'), clip=torch.cat([torch.full((p.num_entries,), c, dtype=torch.int64) for c, p in enumerate(packs)]),
        num_entries=e0[-1], num_focal=sum(p.num_focal for p in packs), time_unit=unit)


def _present_and_speed(raw_data, desired_speed, skip_frames):
    """pack_clip's presence rule and per-agent desired speed of one clip, on the CPU."""
    from .data.data import desired_speed_per_agent
    P = torch.as_tensor(raw_data.position).detach().float().cpu()
    V = torch.as_tensor(raw_data.velocity).detach().float().cpu()
    D = torch.as_tensor(raw_data.destination).detach().float().cpu()
    N = P.shape[1]
    present = torch.isfinite(P).all(-1) & torch.isfinite(V).all(-1) & torch.isfinite(D).all(-1)
    mask_v = getattr(raw_data, 'mask_v', None)
    if mask_v is not None:
        present &= torch.as_tensor(mask_v).cpu() != 0
    if desired_speed is None:
        v0 = desired_speed_per_agent(torch.where(present.unsqueeze(-1), V, torch.zeros_like(V)), skip_frames)
    else:
        v0 = torch.as_tensor(desired_speed, dtype=torch.float32).detach().cpu().reshape(-1)
        v0 = v0.expand(N).clone() if v0.numel() == 1 else v0
        if v0.numel() != N:
            raise ValueError(f'desired_speed must hold N={N} values, got {v0.numel()}')
    return P, V, D, present, v0


ROLL_SMALL = 64           # windows up to this many slots: a lane per slot, states in LDS (with horizon <= ROLL_SMALL_MAX_H)
ROLL_SMALL_MAX_H = 48
PRESENT, INJECTED, CARRIED = 1, 2, 4


def pack_windows(data, horizon, frames=None, stride=1, desired_speed=None, skip_frames=25, device=None):
    """Rollout windows of one or more clips as the rollout-fit kernel reads them, built once per fit.

    data: a `RawData` (a loaded clip or `ScenarioResult.to_raw_data()`) or a list of them; windows never cross clips and
    every clip's time unit must agree.  Presence is pack_clip's rule.  frames: the frame range of every clip (None = all;
    a slice, 'a:b' or a list of consecutive frames).  A window starts at every `stride`-th frame t0 of the range whose
    t0 + horizon is in the range too, and its slots are the agents present in any of its frames t0 .. t0 + horizon,
    ascending.  Entry (w, k, s) = (H + 1) slot_offsets[w] + k n_w + s: `rec` (p, v) recorded in frame t0 + k (0 where
    absent), `destination`, `flags` (PRESENT; INJECTED: present and not in k - 1, or k = 0; CARRIED: present in k and
    k - 1, one loss term).  desired_speed: per clip as pack_clip (a list for several clips, or one scalar for all).
    small_windows / big_windows: windows of <= 64 slots (when horizon <= 48) / the others, with big_base the prefix sum
    of the big windows' slot counts."""
    clips = list(data) if isinstance(data, (list, tuple)) else [data]
    if not clips:
        raise ValueError('no clip to pack')
    H = int(horizon)
    if H < 1:
        raise ValueError(f'horizon must be >= 1, got {horizon}')
    stride = int(stride)
    if stride < 1:
        raise ValueError(f'stride must be >= 1, got {stride}')
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    unit = _clip_time_unit(clips)
    recs, dests, flags, speeds, counts, agents, clip_of, starts = [], [], [], [], [], [], [], []
    for c, (raw, ds) in enumerate(zip(clips, _per_clip(desired_speed, clips, 'desired_speed'))):
        P, V, D, present, v0 = _present_and_speed(raw, ds, skip_frames)
        fl = _frame_list(frames, P.shape[0])
        if fl and fl != list(range(fl[0], fl[0] + len(fl))):
            raise ValueError('the frame range of a rollout fit must be consecutive frames')
        state = torch.where(present.unsqueeze(-1), torch.cat((P, V), -1), torch.zeros(()))
        dest = torch.where(present.unsqueeze(-1), D, torch.zeros(()))
        for s in range(0, len(fl) - H, stride):
            t0 = fl[s]
            pres = present[t0:t0 + H + 1]                                     # (H + 1, N)
            ag = pres.any(0).nonzero(as_tuple=True)[0]
            pw = pres[:, ag]
            prev = torch.cat((torch.zeros(1, len(ag), dtype=torch.bool), pw[:-1]), 0)
            fw = pw.to(torch.uint8) * PRESENT + (pw & ~prev).to(torch.uint8) * INJECTED + (pw & prev).to(torch.uint8) * CARRIED
            recs.append(state[t0:t0 + H + 1, ag].reshape(-1, 4))
            dests.append(dest[t0:t0 + H + 1, ag].reshape(-1, 2))
            flags.append(fw.reshape(-1))
            speeds.append(v0[ag])
            counts.append(len(ag))
            agents.append(ag)
            clip_of.append(c)
            starts.append(t0)
    W = len(counts)
    cnt = torch.tensor(counts, dtype=torch.int64)
    offsets = torch.zeros(W + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(cnt, 0)
    S = int(offsets[-1])
    if (H + 1) * S >= 2 ** 31:
        raise ValueError(f'{(H + 1) * S} window entries: more than the packing indexes (int32)')
    small = (cnt <= ROLL_SMALL) if H <= ROLL_SMALL_MAX_H else torch.zeros(W, dtype=torch.bool)
    w_idx = torch.arange(W, dtype=torch.int64)
    big_cnt = cnt[~small]
    big_base = torch.zeros(len(big_cnt), dtype=torch.int64)
    if len(big_cnt):
        big_base[1:] = torch.cumsum(big_cnt, 0)[:-1]
    fl_all = torch.cat(flags) if flags else torch.zeros(0, dtype=torch.uint8)
    carried = ((fl_all & CARRIED) != 0).reshape(-1)
    # terms per k: the entries of window w are k-major blocks of n_w
    k_of = torch.cat([torch.arange(H + 1).repeat_interleave(n) for n in counts]) if counts else torch.zeros(0, dtype=torch.int64)
    per_k = torch.bincount(k_of[carried], minlength=H + 1)[1:] if counts else torch.zeros(H, dtype=torch.int64)
    i32 = lambda x: x.to(torch.int32).contiguous().to(device)                 # noqa: E731
    f32 = lambda x: x.to(torch.float32).contiguous().to(device)               # noqa: E731
    return types.SimpleNamespace(
        rec=f32(torch.cat(recs) if recs else torch.zeros(0, 4)), destination=f32(torch.cat(dests) if dests else torch.zeros(0, 2)),
        flags=fl_all.contiguous().to(device), desired_speed=f32(torch.cat(speeds) if speeds else torch.zeros(0)),
        slot_offsets=i32(offsets), small_windows=i32(w_idx[small]), big_windows=i32(w_idx[~small]), big_base=i32(big_base),
        big_slots=int(big_cnt.sum()), horizon=H, stride=stride, num_windows=W, num_slots=S,
        num_terms=int(carried.sum()), terms_per_step=per_k.tolist(), slot_count=counts,
        agent=torch.cat(agents) if agents else torch.zeros(0, dtype=torch.int64), clip=clip_of, start=starts,
        time_unit=unit)


def _params_vector(d, device):
    return torch.tensor([float(d[k]) for k in PARAM_NAMES], dtype=torch.float32, device=device)


def mlapm_fit_loss(pack, params, version='GC', dt=None, radius=0.3):
    """(loss, grad) at `params` (a dict of the six constants, or a (6,) device tensor) as Python numbers."""
    from . import ops
    dev = pack.state.device
    p = params if isinstance(params, torch.Tensor) else _params_vector({**DEFAULT_INIT, **params}, dev)
    loss, grad = ops.mlapm_fit_loss_grad(pack, p, version, pack.time_unit if dt is None else dt, radius)
    return float(loss.item()), grad.cpu().tolist()


def mlapm_rollout_fit_loss(pack, params, version='GC', dt=None, radius=0.3, time_decay=1.0, per_step=False):
    """(loss, grad) of the rollout loss on a pack_windows result at `params` (a dict of the six constants, or a (6,)
    device tensor) as Python numbers; with per_step=True also (sse, count), the squared-error sums and term counts of
    k = 1 .. H as lists."""
    from . import ops
    dev = pack.rec.device
    p = params if isinstance(params, torch.Tensor) else _params_vector({**DEFAULT_INIT, **params}, dev)
    ps = torch.empty(2 * pack.horizon, dtype=torch.float64, device=dev) if per_step else None
    loss, grad = ops.mlapm_rollout_fit_loss_grad(pack, p, version, pack.time_unit if dt is None else dt, radius,
                                                 time_decay, per_step=ps)
    if not per_step:
        return float(loss.item()), grad.cpu().tolist()
    ps = ps.cpu().tolist()
    return float(loss.item()), grad.cpu().tolist(), (ps[:pack.horizon], ps[pack.horizon:])


class CalibrationResult(types.SimpleNamespace):
    """params: {'version', 'tau', 'A', 'B', 'C', 'D', 'theta'} -- `MLAPM(**params)` as is; initial_loss / final_loss;
    history: the loss before each optimiser step; steps; fit: the names that were fitted; horizon: None (one-step
    velocity loss) or the rollout length of the position loss.  calibrate_mlapm_to_stats: history is the best objective
    so far per generation, and terms, generations, population, seeds and status are added."""


def calibrate_mlapm(data, version='GC', init=None, fit=PARAM_NAMES, steps=500, lr=0.02, lr_final=0.01, use_graph=True,
                    graph_steps=50, radius=0.3, dt=None, frames=None, desired_speed=None, skip_frames=25, target=None,
                    betas=(0.9, 0.999), eps=1e-12, device=None, horizon=None, stride=1, time_decay=1.0):
    """Fit MLAPM's constants to a clip with Adam on the device.

    data: a RawData or a list of them (packed here with pack_clip(frames, desired_speed, skip_frames, target)) or a
    pack_clip result.
    horizon: None fits the one-step velocity loss above (piml_mlapm_fit_loss_grad).  horizon=H fits the H-step rollout
    loss instead (piml_mlapm_rollout_fit_loss_grad: windows of pack_windows(data, H, frames, stride, desired_speed,
    skip_frames), or a pack_windows result as `data`; positions weighted by time_decay^(H - k)), with the same Adam,
    schedule, masking and capture.
    init: starting constants (default: main_mlapm.py's, DEFAULT_INIT); fit: the names that move, the others stay fixed
    (their gradient is masked).  dt: the clip's time unit by default.
    One iteration = piml_mlapm_fit_loss_grad + an Adam step of the 6-vector, both on the device.  Adam runs on
    x = params / scale with scale = |init| per constant (1 where init is 0), so `lr` is a step size RELATIVE to each
    constant's magnitude -- theta in degrees near 56 and C near 0.2 move alike -- and it decays on a cosine from lr to
    lr * lr_final over `steps` (Adam's steady steps of size ~lr would otherwise keep the fit from settling).
    use_graph: `graph_steps` iterations are captured into ONE graph (a single stream, no branches) and replayed; the
    eager path runs the same launches (hip_graphs_safe() decides, as everywhere in the package).  The two give bitwise
    equal results.  Nothing is read back before the end."""
    from . import ops, hip_graphs_safe
    if version not in ops.MLAPM_VARIANTS:
        raise NotImplementedError(version)
    unknown = [k for k in fit if k not in PARAM_NAMES]
    if unknown:
        raise ValueError(f'unknown constants to fit: {unknown} (of {PARAM_NAMES})')
    if horizon is None:
        pack = data if hasattr(data, 'offsets') else pack_clip(data, frames=frames, desired_speed=desired_speed,
                                                                skip_frames=skip_frames, target=target, device=device)
        ref = pack.state
    else:
        if target is not None:
            raise ValueError('target: the rollout loss fits recorded positions')
        pack = data if hasattr(data, 'slot_offsets') else pack_windows(data, horizon, frames=frames, stride=stride,
                                                                       desired_speed=desired_speed,
                                                                       skip_frames=skip_frames, device=device)
        if int(pack.horizon) != int(horizon):
            raise ValueError(f'the pack holds windows of {pack.horizon} steps, not {horizon}')
        ref = pack.rec
    dev = ref.device
    if not ref.is_cuda:
        raise ValueError('calibrate_mlapm needs the clip packed on a GPU')
    dt = pack.time_unit if dt is None else float(dt)
    if not dt > 0:
        raise ValueError('no time unit: pass dt')
    start = {**DEFAULT_INIT, **(init or {})}
    steps = int(steps)
    with torch.no_grad():
        p0 = torch.tensor([float(start[k]) for k in PARAM_NAMES], dtype=torch.float64, device=dev)
        scale = torch.where(p0 != 0, p0.abs(), torch.ones_like(p0))
        mask = torch.tensor([k in fit for k in PARAM_NAMES], dtype=torch.float64, device=dev)
        x = p0 / scale
        params = p0.float()
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        t = torch.zeros(1, dtype=torch.float64, device=dev)
        t_idx = torch.zeros(1, dtype=torch.long, device=dev)
        loss = torch.empty(1, dtype=torch.float64, device=dev)
        grad = torch.empty(6, dtype=torch.float32, device=dev)
        hist = torch.zeros(max(steps, 1), dtype=torch.float64, device=dev)
        b1, b2 = betas
        one = torch.ones(1, dtype=torch.float64, device=dev)
        if horizon is None:
            loss_grad = lambda **kw: ops.mlapm_fit_loss_grad(pack, params, version, dt, radius, **kw)   # noqa: E731
        else:
            loss_grad = lambda **kw: ops.mlapm_rollout_fit_loss_grad(pack, params, version, dt, radius,  # noqa: E731
                                                                     time_decay, **kw)

        def iteration():
            loss_grad(loss=loss, grad=grad)
            hist.index_copy_(0, t_idx, loss)
            t_idx.add_(1)
            t.add_(1.0)
            g = grad.double() * scale * mask
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            mhat = m / (one - torch.pow(b1, t))
            vhat = v / (one - torch.pow(b2, t))
            frac = torch.clamp(t / max(steps, 1), max=1.0)
            lr_t = lr * (lr_final + (1 - lr_final) * 0.5 * (1 + torch.cos(math.pi * frac)))
            x.sub_(lr_t * mhat / (vhat.sqrt() + eps))
            params.copy_(x * scale)

        loss_grad(loss=loss, grad=grad)                        # also sizes the workspace
        initial = loss.clone()
        done = 0
        per = max(1, int(graph_steps))
        if use_graph and steps >= per + 1 and hip_graphs_safe():
            iteration()                                       # a real iteration, also warms the library up
            done = 1
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(per):
                    iteration()
            for _ in range((steps - done) // per):
                g.replay()
            done += (steps - done) // per * per
        for _ in range(steps - done):
            iteration()
        final, _ = loss_grad()
        out = params.double().cpu().tolist()
    res = {'version': version}
    res.update({k: float(val) for k, val in zip(PARAM_NAMES, out)})
    return CalibrationResult(params=res, initial_loss=float(initial.item()), final_loss=float(final.item()),
                             history=hist[:steps].cpu().tolist(), steps=steps, fit=tuple(fit), horizon=horizon)


OBJECTIVE_KEYS = {'crowd': ('fd_distance', 'map_distance', 'mean_speed_diff'),
                  'pairs': ('ttc_l1', 'nn_l1', 'overlap_rate_diff'),
                  'obstacles': ('hit_track_fraction_diff', 'contact_rate_diff', 'clearance_l1'),
                  'groups': ('group_fraction_diff', 'size_l1', 'member_distance_l1', 'abreast_l1', 'speed_ratio_diff'),
                  'tracks': ('heading_ac_max_diff', 'persistence_time_diff', 'msd_exponent_diff', 'acc_l1',
                             'mean_acceleration_diff', 'straightness_l1', 'speed_l1', 'duration_l1'),
                  'views': ('map_l1', 'nn_map_l1', 'gap_l1', 'front_back_diff', 'passing_side_diff', 'g_map_max_diff',
                            'headway_slope_diff', 'headway_intercept_diff')}
# speed_ratio_diff needs min_count GROUPED tracks on both sides, which a recorded clip does not have (GC 11, UCY 26): NaN at
# any honest min_count, and a NaN term of non-zero weight makes J infinite -- so it is off unless `weights` switches it on
DEFAULT_WEIGHTS = {'speed_ratio_diff': 0.0}
# the track side: persistence_time_diff is NaN for both recorded clips (their heading autocorrelation never falls to 1 / e
# inside the lags); speed_l1 and duration_l1 belong to the scene (the desired speeds and the routes), not the law
TRACK_DEFAULT_WEIGHTS = {'persistence_time_diff': 0.0, 'speed_l1': 0.0, 'duration_l1': 0.0}
# the view side: g_map_max_diff and the headway fit need min_count pairs per cell / agents per gap bin on both sides, which
# a short clip or a small ensemble does not hold -- NaN there, so they are off unless `weights` switches them on
VIEW_DEFAULT_WEIGHTS = {'g_map_max_diff': 0.0, 'headway_slope_diff': 0.0, 'headway_intercept_diff': 0.0}
DEFAULT_BOUNDS = {'tau': (1e-3, None), 'Aw': (0.0, None), 'Bw': (None, 0.0), 'Ag': (0.0, None), 'group_dist': (0.0, None),
                  'An': (0.0, None), 'noise_tau': (0.0, None)}
GROUP_OPTION_KEYS = ('radius', 'dv_max', 'v_min', 'min_time', 'share', 'r_bin', 'r_bins', 'a_bins')


def stats_objective(crowd=None, pairs=None, ref_crowd=None, ref_pairs=None, weights=None, min_count=50, obstacles=None,
                    ref_obstacles=None, groups=None, ref_groups=None, tracks=None, ref_tracks=None, views=None,
                    ref_views=None):
    """(J, terms): how far simulated statistics are from a reference's.  crowd / ref_crowd: CrowdStats, pairs / ref_pairs:
    PairStats, obstacles / ref_obstacles: ObstacleStats, groups / ref_groups: GroupStats, tracks / ref_tracks: TrackStats
    (compare_track_stats' terms, OBJECTIVE_KEYS['tracks']: weight 1.0 for heading_ac_max_diff, msd_exponent_diff, acc_l1,
    mean_acceleration_diff and straightness_l1, 0.0 by default (TRACK_DEFAULT_WEIGHTS) for persistence_time_diff -- NaN for
    both recorded clips -- and for speed_l1 and duration_l1, which belong to the scene, not the law); a side takes part when both of its
    statistics are given.  views / ref_views: ViewStats (compare_view_stats' terms, OBJECTIVE_KEYS['views']: weight 1.0 for
    map_l1, nn_map_l1, gap_l1, front_back_diff and passing_side_diff, 0.0 by default (VIEW_DEFAULT_WEIGHTS) for
    g_map_max_diff and the two headway terms, NaN on short clips).  terms is
    the union of compare_crowd_stats(crowd, ref_crowd, min_count), compare_pair_stats(pairs, ref_pairs, min_count),
    compare_obstacle_stats(obstacles, ref_obstacles, min_count) and compare_group_stats(groups, ref_groups, min_count) for
    the sides given, and
    J = sum_k w_k |terms[k]| over fd_distance, map_distance, mean_speed_diff (crowd), ttc_l1, nn_l1, overlap_rate_diff
    (pairs), hit_track_fraction_diff, contact_rate_diff, clearance_l1 (obstacles) and group_fraction_diff, size_l1,
    member_distance_l1, abreast_l1, speed_ratio_diff (groups), every weight 1.0 unless `weights` names it -- but
    speed_ratio_diff, whose default weight is 0.0 (DEFAULT_WEIGHTS: it needs min_count grouped tracks on both sides, more
    than a recorded clip holds).  map_distance is left out when it is None (no common map); a term of weight zero is skipped
    before it is looked at, and a NaN term of non-zero weight makes J = inf.  ValueError: no side given, or a weight for an
    unknown key."""
    from .crowdstats import compare_crowd_stats
    from .pairstats import compare_pair_stats
    known = OBJECTIVE_KEYS['crowd'] + OBJECTIVE_KEYS['pairs'] + OBJECTIVE_KEYS['obstacles'] + OBJECTIVE_KEYS['groups'] + \
        OBJECTIVE_KEYS['tracks'] + OBJECTIVE_KEYS['views']
    unknown = sorted(set(weights or {}) - set(known))
    if unknown:
        raise ValueError(f'stats_objective: weights for unknown terms {unknown} (of {known})')
    terms, keys = {}, []
    if crowd is not None and ref_crowd is not None:
        terms.update(compare_crowd_stats(crowd, ref_crowd, min_count))
        keys += OBJECTIVE_KEYS['crowd']
    if pairs is not None and ref_pairs is not None:
        terms.update(compare_pair_stats(pairs, ref_pairs, min_count))
        keys += OBJECTIVE_KEYS['pairs']
    if obstacles is not None and ref_obstacles is not None:
        from .obstaclestats import compare_obstacle_stats
        terms.update(compare_obstacle_stats(obstacles, ref_obstacles, min_count))
        keys += OBJECTIVE_KEYS['obstacles']
    if groups is not None and ref_groups is not None:
        from .groupstats import compare_group_stats
        terms.update(compare_group_stats(groups, ref_groups, min_count))
        keys += OBJECTIVE_KEYS['groups']
    if tracks is not None and ref_tracks is not None:
        from .trackstats import compare_track_stats
        terms.update(compare_track_stats(tracks, ref_tracks, min_count))
        keys += OBJECTIVE_KEYS['tracks']
    if views is not None and ref_views is not None:
        from .viewstats import compare_view_stats
        terms.update(compare_view_stats(views, ref_views, min_count))
        keys += OBJECTIVE_KEYS['views']
    if not keys:
        raise ValueError('stats_objective: neither crowd, pair, obstacle, group, track nor view statistics with a reference')
    J = 0.0
    for k in keys:
        w = float((weights or {}).get(k, DEFAULT_WEIGHTS.get(k, TRACK_DEFAULT_WEIGHTS.get(k, VIEW_DEFAULT_WEIGHTS.get(k, 1.0)))))
        if terms[k] is None or w == 0.0:
            continue
        if math.isnan(terms[k]):
            return float('inf'), terms
        J += w * abs(float(terms[k]))
    return J, terms


def _options_of(stats, keys):
    return {k: stats.options[k] for k in keys}


class _StatsEvaluator:
    """calibrate_mlapm_to_stats' objective on the GPU: list of candidate dicts -> list of J, one SweepRun generation each."""

    def __init__(self, scenario, reference, frames, seeds, population, radius, capacity, crowd_kw, pair_kw, weights,
                 min_count, device, obstacle_kw=None, wall_cutoff=None, group_kw=None, components='device', track_kw=None,
                 view_kw=None):
        from . import crowdstats, pairstats
        from .models.mlapm import DEFAULT_WALL_CUTOFF, SweepRun
        self.ref_obstacles = self.ref_groups = self.ref_tracks = self.ref_views = None
        if isinstance(reference, (tuple, list)):
            if len(reference) == 6:                  # (crowd, pairs, obstacles, groups, tracks, views): the view side too
                self.ref_crowd, self.ref_pairs, self.ref_obstacles, self.ref_groups, self.ref_tracks, self.ref_views = \
                    reference
            elif len(reference) == 5:                  # (crowd, pairs, obstacles, groups, tracks): the track side too
                self.ref_crowd, self.ref_pairs, self.ref_obstacles, self.ref_groups, self.ref_tracks = reference
            elif len(reference) == 4:                  # (crowd, pairs, obstacles, groups): the group side takes part too
                self.ref_crowd, self.ref_pairs, self.ref_obstacles, self.ref_groups = reference
            elif len(reference) == 3:                # (crowd, pairs, obstacles): the obstacle side takes part
                self.ref_crowd, self.ref_pairs, self.ref_obstacles = reference
            else:
                self.ref_crowd, self.ref_pairs = reference
            if obstacle_kw is None and self.ref_obstacles is not None:
                obstacle_kw = _options_of(self.ref_obstacles, ('dt', 'radius', 'hit_radius', 'r_bin', 'r_bins', 'tau_bin',
                                                               'tau_bins', 'box'))
            if group_kw is None and self.ref_groups is not None:
                group_kw = _options_of(self.ref_groups, GROUP_OPTION_KEYS)
            if track_kw is None and self.ref_tracks is not None:
                from .trackstats import OPTION_KEYS as TRACK_OPTION_KEYS
                track_kw = _options_of(self.ref_tracks, [k for k in TRACK_OPTION_KEYS if k != 'dt'])
            if view_kw is None and self.ref_views is not None:
                from .viewstats import OPTION_KEYS as VIEW_OPTION_KEYS
                view_kw = _options_of(self.ref_views, VIEW_OPTION_KEYS)
            if crowd_kw is None and self.ref_crowd is not None:
                crowd_kw = crowdstats.call_options(self.ref_crowd)
            if pair_kw is None and self.ref_pairs is not None:
                pair_kw = _options_of(self.ref_pairs, ('radius', 'lags', 'tau_bin', 'tau_bins', 'r_bin', 'r_bins', 'r_max',
                                                       'box'))
        else:                                     # a RawData: its own statistics, the crowd box its bounding box
            crowd_kw = dict(crowd_kw or {})
            if crowd_kw.get('box') is None:
                crowd_kw['box'] = crowdstats.auto_box(torch.as_tensor(reference.position).cpu().numpy(),
                                                      torch.as_tensor(reference.mask_p).cpu().numpy(),
                                                      crowd_kw.get('cell', 0.5))
            self.ref_crowd = crowdstats.crowd_stats_of_raw(reference, **crowd_kw)
            self.ref_pairs = pairstats.pair_stats_of_raw(reference, **dict(pair_kw or {}))
            if frames is None:
                frames = int(torch.as_tensor(reference.position).shape[0])
        if self.ref_crowd is None and self.ref_pairs is None and self.ref_obstacles is None and self.ref_groups is None and \
                self.ref_tracks is None and self.ref_views is None:
            raise ValueError('calibrate_mlapm_to_stats: the reference holds no statistics')
        self.crowd_kw, self.pair_kw, self.obstacle_kw = dict(crowd_kw or {}), dict(pair_kw or {}), dict(obstacle_kw or {})
        self.group_kw, self.components, self.track_kw = dict(group_kw or {}), components, dict(track_kw or {})
        self.view_kw = dict(view_kw or {})
        self.weights, self.min_count, self.radius = weights, min_count, radius
        self.frames = 200 if frames is None else int(frames)
        self.run = SweepRun(scenario, self.frames, population, seeds, capacity=capacity, device=device,
                            wall_cutoff=DEFAULT_WALL_CUTOFF if wall_cutoff is None else wall_cutoff)
        self.seconds = {'run': 0.0, 'crowd': 0.0, 'pairs': 0.0, 'obstacles': 0.0, 'groups': 0.0, 'tracks': 0.0, 'host': 0.0}
        if self.ref_views is not None:
            self.seconds['views'] = 0.0
        self.last_terms = []

    def __call__(self, cands):
        import time
        t0 = time.perf_counter()
        sw = self.run.run(cands, self.radius)
        # one reduction: a member with a non-finite position or velocity in a present slot is an exploded run
        bad = ((~(torch.isfinite(sw.position).all(-1) & torch.isfinite(sw.velocity).all(-1))) & (sw.mask_p != 0)) \
            .flatten(1).any(1)
        bad_host = bad.cpu().tolist()                                         # (synchronises: the run is done)
        t1 = time.perf_counter()
        mask = sw.mask_p
        if any(bad_host):                          # never hand an exploded member to the statistics kernels as it is
            mask = mask.clone()
            mask[bad] = 0.0
        n_active = [min(int(n), sw.capacity) for n in sw.spawned]
        crowd = pairs = None
        if self.ref_crowd is not None:
            from .crowdstats import crowd_stats
            crowd = crowd_stats(sw.position, sw.velocity, mask, n_active=n_active, **self.crowd_kw)
        t2 = time.perf_counter()
        if self.ref_pairs is not None:
            from .pairstats import pair_stats
            pairs = pair_stats(sw.position, sw.velocity, mask, n_active=n_active, **self.pair_kw)
        t3 = time.perf_counter()
        obstacles = None
        if self.ref_obstacles is not None:           # the scene's own obstacle statistics, one call for all members
            from .obstaclestats import obstacle_stats
            kw = {'dt': float(sw.time_unit), **self.obstacle_kw}
            obstacles = obstacle_stats(sw.position, sw.velocity, mask, sw.obstacles, n_active=n_active, **kw)
        t3b = time.perf_counter()
        groups = None
        if self.ref_groups is not None:              # one call for every member: both passes and the components between them
            from .groupstats import group_stats
            kw = {'dt': float(sw.time_unit), **self.group_kw}
            groups = group_stats(sw.position, mask, n_active=n_active, components=self.components, **kw)
        t3c = time.perf_counter()
        tracks = None
        if self.ref_tracks is not None:              # one call for every member, the reference's options, the scene's dt
            from .trackstats import track_stats
            kw = {'dt': float(sw.time_unit), **self.track_kw}
            tracks = track_stats(sw.position, mask, n_active=n_active, **kw)
        t3d = time.perf_counter()
        views = None
        if self.ref_views is not None:               # one call for every member and lag, the reference's options
            from .viewstats import view_stats
            views = view_stats(sw.position, sw.velocity, mask, n_active=n_active, **self.view_kw)
            self.seconds['views'] += time.perf_counter() - t3d
        t3e = time.perf_counter()
        out, self.last_terms = [], []
        for c in range(sw.n_candidates):
            group = sw.members_of(c)
            if any(bad_host[m] for m in group):
                out.append(float('inf'))
                self.last_terms.append({'exploded': True})
                continue
            J, terms = stats_objective(None if crowd is None else crowd.select(group).pooled(),
                                       None if pairs is None else pairs.select(group).pooled(),
                                       self.ref_crowd, self.ref_pairs, self.weights, self.min_count,
                                       None if obstacles is None else obstacles.select(group).pooled(), self.ref_obstacles,
                                       None if groups is None else groups.select(group).pooled(), self.ref_groups,
                                       None if tracks is None else tracks.select(group).pooled(), self.ref_tracks,
                                       None if views is None else views.select(group).pooled(), self.ref_views)
            out.append(J)
            self.last_terms.append(terms)
        t4 = time.perf_counter()
        for k, dt in zip(('run', 'crowd', 'pairs', 'obstacles', 'groups', 'tracks', 'host'),
                         (t1 - t0, t2 - t1, t3 - t2, t3b - t3, t3c - t3b, t3d - t3c, t4 - t3e)):
            self.seconds[k] += dt
        return out


def calibrate_mlapm_to_stats(scenario, reference, version='GC', init=None, fit=PARAM_NAMES, frames=None, seeds=range(8),
                             population=16, generations=30, elite=0.25, sigma=0.2, sigma_floor=1e-3, bounds=None,
                             weights=None, crowd_kw=None, pair_kw=None, search_seed=0, radius=0.3, capacity=None,
                             evaluate=None, min_count=50, device='cuda', obstacle_kw=None, wall_cutoff=None, group_kw=None,
                             track_kw=None, view_kw=None):
    """Fit MLAPM's constants so that the law, run open-world in `scenario`, reproduces the reference's crowd statistics.

    The view side: a reference 6-tuple (CrowdStats | None, PairStats | None, ObstacleStats | None, GroupStats | None,
    TrackStats | None, ViewStats | None) adds the heading-frame statistics, the side that sees the law's anisotropy (theta,
    C, D): one view_stats call (view_kw, default the reference's viewstats.OPTION_KEYS options) covers every member and lag
    of a generation and enters stats_objective with the reference's; `seconds` then has a 'views' entry.

    The fluctuation term: fit may also name An, noise_tau (NOISE_PARAM_NAMES), and init may carry them: the candidates then
    run the frames with the fluctuation term (MLAPM(..., An=, noise_tau=)), in any scene.  init must hold An when either is
    fitted or present -- the term has no default -- and noise_tau defaults to 0 (white noise); An >= 0 and noise_tau >= 0
    are bounded so by default.  A reference 5-tuple (CrowdStats | None, PairStats | None, ObstacleStats | None, GroupStats |
    None, TrackStats | None) adds the track side, the one that sees the term: one track_stats call (track_kw, default the
    reference's OPTION_KEYS options; dt the scene's) covers every member of a generation and enters stats_objective with the
    reference's.  The result's params then carry An and noise_tau.

    The group term: fit may also name Ag, group_dist (GROUP_PARAM_NAMES), and init may carry them: the candidates then run a
    grouped clip scene (scenarios.clip_scenario(groups=); ValueError before anything is launched for any other scene) with
    the group term (MLAPM(..., Ag=, group_dist=)).  init must hold Ag when either is fitted or present -- the term has no
    default; about 3 m/s^2 (Moussaid et al. 2010) is a starting point -- and group_dist defaults to 0.5; Ag >= 0 and
    group_dist >= 0 are bounded so by default.  A reference 4-tuple (CrowdStats | None, PairStats | None, ObstacleStats |
    None, GroupStats | None) adds the group side: one group_stats call (group_kw, default the reference's radius, dv_max,
    v_min, min_time, share and bins; dt the scene's; the components on the device) covers every member of a
    generation and enters stats_objective with the reference's.  The result's params then carry Ag and group_dist.

    The wall term: fit may also name Aw, Bw (WALL_PARAM_NAMES), and init may carry Aw, Bw: the candidates then run the
    frames with the wall term (MLAPM(..., Aw=, Bw=, wall_cutoff=wall_cutoff), default cutoff 2.0 m; the cutoff is the
    grid's and is not fitted).  init must hold both when either is fitted -- the term has no default; Aw = 50, Bw = -5
    (Helbing and Molnar 1995) is the literature's starting point -- and Aw >= 0, Bw <= 0 are bounded so by default.  A
    reference triple (CrowdStats | None, PairStats | None, ObstacleStats | None) adds the obstacle side: the candidates'
    obstacle_stats against the scene's own obstacles (obstacle_kw, default the reference's options; one call for every
    member) enter stats_objective with the reference's.  The result's params then carry Aw, Bw and wall_cutoff.

    reference: a RawData (its crowd_stats / pair_stats are taken with crowd_kw / pair_kw, the crowd box defaulting to
    crowdstats.auto_box of the recording, and the simulated side uses the same options, so the maps are comparable) or a
    pair (CrowdStats | None, PairStats | None) (a None side takes no part; the simulated side then uses the reference's
    own options unless crowd_kw / pair_kw are given).  frames: the simulated frames (default: the recording's length, 200
    for a statistics pair).  The objective of a candidate is stats_objective of its members' statistics pooled over
    `seeds` (weights, min_count).
    The search is a cross-entropy method, deterministic under numpy.random.default_rng(search_seed), in calibrate_mlapm's
    scaled space x = p / scale, scale = |init| (1 where init is 0): only the `fit` names move, the other constants are
    carried through bit for bit.  Every generation evaluates `population` candidates -- candidate 0 is the best seen so
    far (generation 0: init), the others mean + sigma z per coordinate, clipped to bounds ({name: (lo, hi)}, None = open;
    tau >= 1e-3 unless overridden) -- and then the mean becomes that of the best ceil(elite * population) candidates with a
    finite objective and the per-coordinate sigma their RMS distance from the previous mean (never below sigma_floor).  A generation is ONE ensemble run of population
    x len(seeds) members: the candidates' law table is overwritten in place, the captured frames are replayed from an
    emptied state (models.mlapm.SweepRun), one crowd_stats and one pair_stats call cover every member, and a candidate
    with a non-finite position or velocity in a present slot of any of its members gets J = inf (its members reach the
    statistics kernels with their masks zeroed).
    evaluate: a callable list[dict] -> list[float] that replaces the simulation (the search then makes no GPU call;
    scenario and reference may be None).
    Not a gradient method (arrivals and retirements are not differentiable); the result is tuned to the chosen seeds
    (common random numbers), and is identified no better than the statistics allow.
    Returns a CalibrationResult: params, initial_loss (init's objective), final_loss, history (the best objective so far
    after each generation, non-increasing), fit, terms (the best candidate's term dict; None with `evaluate`),
    generations, population, seeds, status ('ok', or that no candidate had a finite objective and init was kept)."""
    import numpy as np
    from . import ops
    if version not in ops.MLAPM_VARIANTS:
        raise NotImplementedError(version)
    fit = tuple(fit)
    every = PARAM_NAMES + WALL_PARAM_NAMES + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES
    unknown = [k for k in fit if k not in every]
    if unknown or not fit:
        raise ValueError(f'constants to fit: names of {every} expected, got {fit}')
    walls = any(k in (init or {}) for k in WALL_PARAM_NAMES)
    if (walls or any(k in WALL_PARAM_NAMES for k in fit)) and not all(k in (init or {}) for k in WALL_PARAM_NAMES):
        raise ValueError(f'the wall term has no default: init must hold both of {WALL_PARAM_NAMES} (fit {fit}, init '
                         f'{sorted(init or {})})')
    grouped = any(k in (init or {}) for k in GROUP_PARAM_NAMES)
    if (grouped or any(k in GROUP_PARAM_NAMES for k in fit)) and 'Ag' not in (init or {}):
        raise ValueError(f'the group term has no default: init must hold Ag (fit {fit}, init {sorted(init or {})})')
    noisy = any(k in (init or {}) for k in NOISE_PARAM_NAMES)
    if (noisy or any(k in NOISE_PARAM_NAMES for k in fit)) and 'An' not in (init or {}):
        raise ValueError(f'the fluctuation term has no default: init must hold An (fit {fit}, init {sorted(init or {})})')
    names = PARAM_NAMES + (WALL_PARAM_NAMES if walls else ()) + (GROUP_PARAM_NAMES if grouped else ()) + \
        (NOISE_PARAM_NAMES if noisy else ())
    population, generations = int(population), int(generations)
    if population < 2 or generations < 1:
        raise ValueError(f'population >= 2 and generations >= 1 expected, got {population}, {generations}')
    if not 0 < float(elite) <= 1 or not float(sigma) > 0 or not float(sigma_floor) >= 0:
        raise ValueError(f'elite in (0, 1], sigma > 0, sigma_floor >= 0 expected, got {elite}, {sigma}, {sigma_floor}')
    bad = sorted(set(bounds or {}) - set(every))
    if bad:
        raise ValueError(f'bounds for unknown constants {bad}')
    limits = {**DEFAULT_BOUNDS, **(bounds or {})}
    start = {**DEFAULT_INIT, **(init or {})}
    if grouped:
        from .models.mlapm import DEFAULT_GROUP_DIST, check_scene_groups, group_args
        start.setdefault('group_dist', DEFAULT_GROUP_DIST)
        group_args({k: start[k] for k in GROUP_PARAM_NAMES})
        if scenario is not None:
            check_scene_groups(scenario)
    if noisy:
        from .models.mlapm import DEFAULT_NOISE_TAU, noise_args
        start.setdefault('noise_tau', DEFAULT_NOISE_TAU)
        noise_args({k: start[k] for k in NOISE_PARAM_NAMES})
    start = {k: float(start[k]) for k in names}
    if walls:
        from .models.mlapm import DEFAULT_WALL_CUTOFF, wall_args
        wall_cutoff = DEFAULT_WALL_CUTOFF if wall_cutoff is None else float(wall_cutoff)
        wall_args({'Aw': start['Aw'], 'Bw': start['Bw'], 'wall_cutoff': wall_cutoff})
    seeds = [int(x) for x in seeds]
    terms_of = None
    if evaluate is None:
        evaluate = terms_of = _StatsEvaluator(scenario, reference, frames, seeds, population, radius, capacity, crowd_kw,
                                              pair_kw, weights, min_count, device, obstacle_kw, wall_cutoff, group_kw,
                                              track_kw=track_kw, view_kw=view_kw)
    scale = np.array([abs(start[k]) if start[k] != 0 else 1.0 for k in fit])
    lo = np.array([-np.inf if limits.get(k, (None, None))[0] is None else limits[k][0] for k in fit], np.float64)
    hi = np.array([np.inf if limits.get(k, (None, None))[1] is None else limits[k][1] for k in fit], np.float64)
    rng = np.random.default_rng(search_seed)
    x_of = lambda p: np.array([p[k] for k in fit]) / scale                    # noqa: E731
    mean, sig = x_of(start), np.full(len(fit), float(sigma))
    n_elite = int(math.ceil(float(elite) * population))
    best, best_J, best_terms, initial, history = dict(start), float('inf'), None, None, []
    for g in range(generations):
        cands = [dict(best)]
        for _ in range(population - 1):
            p = np.clip((mean + sig * rng.standard_normal(len(fit))) * scale, lo, hi)
            cands.append({**start, **{k: float(v) for k, v in zip(fit, p)}})
        J = [float(v) for v in evaluate([{'version': version, **c} for c in cands])]
        if len(J) != population:
            raise ValueError(f'evaluate returned {len(J)} values for {population} candidates')
        J = [v if math.isfinite(v) else float('inf') for v in J]              # NaN and inf are never selected
        if g == 0:
            initial = J[0]
        order = sorted((i for i in range(population) if math.isfinite(J[i])), key=lambda i: (J[i], i))
        if order and J[order[0]] < best_J:
            best, best_J = dict(cands[order[0]]), J[order[0]]
            if terms_of is not None:
                best_terms = terms_of.last_terms[order[0]]
        if order:
            xs = np.stack([x_of(cands[i]) for i in order[:n_elite]])
            # sigma about the OLD mean (the rank-mu form): while the elite sits to one side of the mean the spread keeps the
            # length of the move instead of collapsing onto the elite's own scatter, which stalls a plain cross-entropy
            # update well short of an optimum several sigma away
            sig = np.maximum(np.sqrt(((xs - mean) ** 2).mean(0)), float(sigma_floor))
            mean = xs.mean(0)
        history.append(best_J)
    status = 'ok' if math.isfinite(best_J) else 'no candidate had a finite objective: init kept'
    if status != 'ok':
        import warnings
        warnings.warn(f'calibrate_mlapm_to_stats: {status}')
    res = {'version': version, **best}
    if walls:
        res['wall_cutoff'] = wall_cutoff
    out = CalibrationResult(params=res, initial_loss=initial, final_loss=best_J, history=history, fit=fit,
                            terms=best_terms, generations=generations, population=population, seeds=seeds, status=status,
                            steps=generations, horizon=None)
    if terms_of is not None:
        out.seconds = dict(terms_of.seconds)
    return out


def _parse_init(text):
    out = {}
    for item in filter(None, (s.strip() for s in (text or '').split(','))):
        k, _, val = item.partition('=')
        if k not in PARAM_NAMES + WALL_PARAM_NAMES + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES or not _:
            raise argparse.ArgumentTypeError('--init expects name=value with names in '
                                             f'{PARAM_NAMES + WALL_PARAM_NAMES + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES}, got {item!r}')
        out[k] = float(val)
    return out


def _parse_fit(text):
    names = tuple(filter(None, (s.strip() for s in text.split(','))))
    bad = [k for k in names if k not in PARAM_NAMES + WALL_PARAM_NAMES + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES]
    if bad or not names:
        raise argparse.ArgumentTypeError(f'--fit expects names from {PARAM_NAMES + WALL_PARAM_NAMES + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES}, '
                                         f'got {text!r}')
    return names


def get_args(argv=None):
    p = argparse.ArgumentParser(description="fit MLAPM's constants (tau, A, B, C, D, theta) to a clip on the GPU")
    p.add_argument('--data', type=str, nargs='+', required=True,
                   help='one or more v2.2 clips (.npy), recorded or written by piml_amd.simulate')
    p.add_argument('--version', type=str, default='GC', choices=['raw', 'GC', 'UCY'])
    p.add_argument('--init', type=_parse_init, default={}, help='starting constants, e.g. A=7.55,B=-3 (default: main_mlapm.py\'s)')
    p.add_argument('--fit', type=_parse_fit, default=PARAM_NAMES, help='constants to fit, e.g. A,B,theta (default: all six)')
    p.add_argument('--frames', type=str, default=None, help='training frames a:b (default: all)')
    p.add_argument('--valid_frames', type=str, default=None, help='held-out frames c:d: their loss is reported before and after')
    p.add_argument('--horizon', type=int, default=None,
                   help='fit H-step closed-loop rollouts (position error) instead of one step (velocity error)')
    p.add_argument('--stride', type=int, default=1, help='rollout windows start every this many frames')
    p.add_argument('--time_decay', type=float, default=1.0, help='rollout step k weighs time_decay^(H - k)')
    p.add_argument('--steps', type=int, default=500)
    p.add_argument('--lr', type=float, default=0.02, help='Adam step size relative to each constant\'s magnitude')
    p.add_argument('--radius', type=float, default=0.3)
    p.add_argument('--skip_frames', type=int, default=25, help='desired speed = mean |v| over this many frames after the start')
    p.add_argument('--no_graph', action='store_true', help='eager iterations instead of a replayed graph')
    p.add_argument('--out', type=str, default='params.json')
    p.add_argument('--match-stats', dest='match_stats', action='store_true',
                   help="fit the law to the clip's crowd statistics, run open-world in the clip's own scene "
                        '(calibrate_mlapm_to_stats), instead of to its trajectories')
    p.add_argument('--match', type=str, default=None,
                   help='--match-stats: the statistics to match (crowd, pairs, obstacles, groups, tracks, views); default crowd,pairs, '
                        'obstacles too when the law has a wall term (--init Aw=..,Bw=..) and groups too when it has a group '
                        'term (--init Ag=..) and tracks too when it has a fluctuation term (--init An=..)')
    p.add_argument('--scene-groups', dest='scene_groups', type=str, default=None,
                   help="--match-stats: the clip's groups as arrival units, 'auto' (found by groupstats) or a JSON file of "
                        'lists of track indices (simulate --scene-groups); needed by a group term')
    p.add_argument('--wall-cutoff', dest='wall_cutoff', type=float, default=None,
                   help='--match-stats with a wall term: its cutoff in metres (default 2.0); not fitted')
    p.add_argument('--stats-density', dest='stats_density', choices=('gaussian', 'voronoi'), default='gaussian',
                   help='--match-stats: the local density of the crowd statistics (DESIGN 4.16 / 4.20)')
    p.add_argument('--stats-cutoff', dest='stats_cutoff', type=float, default=None,
                   help='--stats-density voronoi: the cut-off radius of a cell (default 1.0)')
    p.add_argument('--scene-frames', dest='scene_frames', type=str, default=None,
                   help="--match-stats: the window 'a:b' of the clip that is the scene and the reference (default: all)")
    p.add_argument('--scene-jitter', dest='scene_jitter', type=float, default=0.0,
                   help='--match-stats: arrivals start within +- this many metres of the recorded origin')
    p.add_argument('--seeds', type=str, default='0:8', help="--match-stats: the seeds every candidate runs, 'a:b' or 'a,b,c'")
    p.add_argument('--population', type=int, default=16)
    p.add_argument('--generations', type=int, default=30)
    p.add_argument('--search-seed', dest='search_seed', type=int, default=0)
    a = p.parse_args(argv)
    wall_names = [k for k in WALL_PARAM_NAMES if k in a.init or k in a.fit]
    if wall_names:
        if not a.match_stats:
            p.error(f'{wall_names}: the wall term is fitted by --match-stats only (it exists in the scene runs, not in the '
                    'one-step or rollout fit)')
        if not all(k in a.init for k in WALL_PARAM_NAMES):
            p.error('the wall term has no default: --init must give Aw and Bw (the literature starts at Aw=50,Bw=-5)')
    elif a.wall_cutoff is not None:
        p.error('--wall-cutoff needs a wall term (--init Aw=..,Bw=..)')
    group_names = [k for k in GROUP_PARAM_NAMES if k in a.init or k in a.fit]
    if group_names:
        if not a.match_stats:
            p.error(f'{group_names}: the group term is fitted by --match-stats only (it exists in the scene runs, not in the '
                    'one-step or rollout fit)')
        if 'Ag' not in a.init:
            p.error('the group term has no default: --init must give Ag (the literature starts at Ag=3)')
        if a.scene_groups is None:
            p.error("the group term needs the clip's groups: --scene-groups auto or FILE.json")
    noise_names = [k for k in NOISE_PARAM_NAMES if k in a.init or k in a.fit]
    if noise_names:
        if not a.match_stats:
            p.error(f'{noise_names}: the fluctuation term is fitted by --match-stats only (it exists in the scene runs, not '
                    'in the one-step or rollout fit)')
        if 'An' not in a.init:
            p.error('the fluctuation term has no default: --init must give An (m/s^2, e.g. An=0.5)')
    if a.scene_groups is not None and not a.match_stats:
        p.error('--scene-groups belongs to --match-stats')
    if a.match_stats:
        if len(a.data) != 1:
            p.error('--match-stats takes one clip')
        if a.match is None:
            a.match = ('crowd,pairs,obstacles' if wall_names else 'crowd,pairs') + (',groups' if group_names else '') + \
                (',tracks' if noise_names else '')
        a.match = tuple(filter(None, (x.strip() for x in a.match.split(','))))
        if not a.match or any(x not in ('crowd', 'pairs', 'obstacles', 'groups', 'tracks', 'views') for x in a.match):
            p.error(f"--match: 'crowd', 'pairs', 'obstacles', 'groups', 'tracks', 'views' or several expected, got {a.match}")
        if a.scene_groups is not None and a.scene_groups != 'auto':
            try:
                from .simulate import load_scene_groups
                a.scene_groups = load_scene_groups(a.scene_groups)
            except (OSError, ValueError) as ex:
                p.error(f'--scene-groups: {ex}')
        try:
            from .crowdstats import check_density
            check_density(a.stats_density, a.stats_cutoff)
        except ValueError as ex:
            p.error(f'--stats-density / --stats-cutoff: {ex}')
        try:
            from .simulate import parse_seeds
            a.seeds = parse_seeds(a.seeds)
            if a.scene_frames is not None:
                lo, hi = (int(x) for x in a.scene_frames.split(':'))
                a.scene_frames = (lo, hi)
        except ValueError as ex:
            p.error(f'--seeds / --scene-frames: {ex}')
    return a


def main(argv=None):
    a = get_args(argv)
    from .data.data import RawData
    raws = []
    for path in a.data:
        raw = RawData()
        raw.load_trajectory_data(path)
        raws.append(raw)
    raw = raws[0] if len(raws) == 1 else raws
    init = {**DEFAULT_INIT, **a.init}
    if a.match_stats:
        return _main_stats(a, raw, init)
    if a.horizon is not None:
        return _main_rollout(a, raw, init)
    pack = pack_clip(raw, frames=a.frames, skip_frames=a.skip_frames)
    res = calibrate_mlapm(pack, version=a.version, init=init, fit=a.fit, steps=a.steps, lr=a.lr, radius=a.radius,
                          use_graph=not a.no_graph)
    print(f'[calibrate] {a.version} on {len(pack.frames)} frames, {pack.num_focal} agent steps: loss {res.initial_loss:.6g} -> '
          f'{res.final_loss:.6g} after {res.steps} steps')
    print('[calibrate] ' + ', '.join(f'{k}={res.params[k]:.6g}' for k in PARAM_NAMES))
    if a.valid_frames:
        vp = pack_clip(raw, frames=a.valid_frames, skip_frames=a.skip_frames)
        before, _ = mlapm_fit_loss(vp, init, a.version, radius=a.radius)
        after, _ = mlapm_fit_loss(vp, res.params, a.version, radius=a.radius)
        print(f'[calibrate] held-out loss ({len(vp.frames)} frames, {vp.num_focal} agent steps): {before:.6g} -> {after:.6g}')
    with open(a.out, 'w') as fh:
        json.dump(res.params, fh, indent=1)
    print(f'[calibrate] wrote {a.out}')
    return res


def _main_rollout(a, raw, init):
    pack = pack_windows(raw, a.horizon, frames=a.frames, stride=a.stride, skip_frames=a.skip_frames)
    res = calibrate_mlapm(pack, version=a.version, init=init, fit=a.fit, steps=a.steps, lr=a.lr, radius=a.radius,
                          use_graph=not a.no_graph, horizon=a.horizon, time_decay=a.time_decay)
    print(f'[calibrate] {a.version} on {pack.num_windows} windows of {a.horizon} steps, {pack.num_terms} agent steps: '
          f'rollout loss {res.initial_loss:.6g} -> {res.final_loss:.6g} m^2 after {res.steps} steps')
    print('[calibrate] ' + ', '.join(f'{k}={res.params[k]:.6g}' for k in PARAM_NAMES))
    if a.valid_frames:
        vp = pack_windows(raw, a.horizon, frames=a.valid_frames, stride=a.stride, skip_frames=a.skip_frames)
        out = []
        for prm in (init, res.params):
            loss, _, (sse, cnt) = mlapm_rollout_fit_loss(vp, prm, a.version, radius=a.radius, time_decay=a.time_decay,
                                                         per_step=True)
            out.append((loss, math.sqrt(sse[-1] / cnt[-1]) if cnt[-1] else float('nan')))
        print(f'[calibrate] held-out rollout loss ({vp.num_windows} windows, {vp.num_terms} agent steps): '
              f'{out[0][0]:.6g} -> {out[1][0]:.6g} m^2; RMSE at k = {a.horizon}: {out[0][1]:.4g} -> {out[1][1]:.4g} m')
    with open(a.out, 'w') as fh:
        json.dump(res.params, fh, indent=1)
    print(f'[calibrate] wrote {a.out}')
    return res


def _main_stats(a, raw, init):
    from . import crowdstats, pairstats, scenarios
    try:
        group_kw = {} if a.scene_groups is None else {'groups': a.scene_groups}
        scene = scenarios.clip_scenario(raw, frames=a.scene_frames, jitter=a.scene_jitter, **group_kw)
    except ValueError as ex:
        sys.exit(f'--match-stats: {ex}')
    lo, hi = a.scene_frames or (0, int(raw.position.shape[0]))
    box = crowdstats.auto_box(raw.position[lo:hi].numpy(), raw.mask_p[lo:hi].numpy(), 0.5)
    density_kw = {} if a.stats_density == 'gaussian' else dict(density=a.stats_density, cutoff=a.stats_cutoff)
    ref_crowd = crowdstats.crowd_stats_of_raw(raw, box=box, frames=(lo, hi), **density_kw) if 'crowd' in a.match else None
    if ref_crowd is not None:
        crowdstats.print_dropped(ref_crowd, 'calibrate --match-stats')
    ref_pairs = pairstats.pair_stats_of_raw(raw, frames=(lo, hi)) if 'pairs' in a.match else None
    ref_obstacles = None
    if 'obstacles' in a.match:
        from . import obstaclestats
        try:
            ref_obstacles = obstaclestats.obstacle_stats_of_raw(raw, scene.obstacles, frames=(lo, hi))
        except ValueError as ex:
            sys.exit(f'--match obstacles: {ex}')
    ref_groups = None
    if 'groups' in a.match:
        from .groupstats import group_stats_of_raw
        ref_groups = group_stats_of_raw(raw, frames=(lo, hi))
    ref_tracks = None
    if 'tracks' in a.match:
        from .trackstats import track_stats_of_raw
        ref_tracks = track_stats_of_raw(raw, frames=(lo, hi))
    reference = (ref_crowd, ref_pairs, ref_obstacles, ref_groups, ref_tracks)
    if 'views' in a.match:
        from .viewstats import view_stats_of_raw
        reference += (view_stats_of_raw(raw, frames=(lo, hi)),)
    res = calibrate_mlapm_to_stats(scene, reference, version=a.version, init=init, fit=a.fit,
                                   frames=hi - lo, seeds=a.seeds, population=a.population, generations=a.generations,
                                   search_seed=a.search_seed, radius=a.radius, wall_cutoff=a.wall_cutoff)
    print(f'[calibrate] {a.version} against the statistics ({", ".join(a.match)}) of frames {lo}:{hi}, {a.population} '
          f'candidates x {len(a.seeds)} seeds x {a.generations} generations: objective {res.initial_loss:.6g} -> '
          f'{res.final_loss:.6g} ({res.status})')
    print('[calibrate] ' + ', '.join(f'{k}={res.params[k]:.6g}' for k in PARAM_NAMES + WALL_PARAM_NAMES + ('wall_cutoff',) + GROUP_PARAM_NAMES + NOISE_PARAM_NAMES
                                     if k in res.params))
    print('[calibrate] terms: ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}'
                                           for k, v in (res.terms or {}).items()))
    with open(a.out, 'w') as fh:
        json.dump(res.params, fh, indent=1)
    print(f'[calibrate] wrote {a.out}')
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
