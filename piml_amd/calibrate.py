"""Calibrate MLAPM's constants (tau, A, B, C, D, theta) to a clip on the GPU.

    python -m piml_amd.calibrate --data clip.npy --version GC [--init A=7.55,B=-3] [--fit A,B,theta] [--frames a:b]
                                 [--valid_frames c:d] [--steps N] --out params.json

The clip is a recorded GC / UCY clip, or one that `python -m piml_amd.simulate` wrote with a trained PINNSF: fitting the
closed-form law to the network's own trajectories distils it into MLAPM's six constants.  The loss is the mean squared
residual of one MLAPM.step per (frame, agent) against the agent's velocity in the next frame, and its gradient with
respect to the constants is analytic (piml_mlapm_fit_loss_grad, one pass over the pairs).  `MLAPM(**result.params)`
simulates with the result."""
import argparse
import json
import math
import os
import sys
import types

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')      # before torch brings the HIP runtime up (piml_amd.hip_graphs_safe)

import torch  # noqa: E402

PARAM_NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
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

    raw_data: a `RawData` (loaded clip, or `ScenarioResult.to_raw_data()`).  An agent is present in frame t when its
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


def _params_vector(d, device):
    return torch.tensor([float(d[k]) for k in PARAM_NAMES], dtype=torch.float32, device=device)


def mlapm_fit_loss(pack, params, version='GC', dt=None, radius=0.3):
    """(loss, grad) at `params` (a dict of the six constants, or a (6,) device tensor) as Python numbers."""
    from . import ops
    dev = pack.state.device
    p = params if isinstance(params, torch.Tensor) else _params_vector({**DEFAULT_INIT, **params}, dev)
    loss, grad = ops.mlapm_fit_loss_grad(pack, p, version, pack.time_unit if dt is None else dt, radius)
    return float(loss.item()), grad.cpu().tolist()


class CalibrationResult(types.SimpleNamespace):
    """params: {'version', 'tau', 'A', 'B', 'C', 'D', 'theta'} -- `MLAPM(**params)` as is; initial_loss / final_loss;
    history: the loss before each optimiser step; steps; fit: the names that were fitted."""


def calibrate_mlapm(data, version='GC', init=None, fit=PARAM_NAMES, steps=500, lr=0.02, lr_final=0.01, use_graph=True,
                    graph_steps=50, radius=0.3, dt=None, frames=None, desired_speed=None, skip_frames=25, target=None,
                    betas=(0.9, 0.999), eps=1e-12, device=None):
    """Fit MLAPM's constants to a clip with Adam on the device.

    data: a RawData (packed here with pack_clip(frames, desired_speed, skip_frames, target)) or a pack_clip result.
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
    pack = data if hasattr(data, 'offsets') else pack_clip(data, frames=frames, desired_speed=desired_speed,
                                                            skip_frames=skip_frames, target=target, device=device)
    dev = pack.state.device
    if not pack.state.is_cuda:
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

        def iteration():
            ops.mlapm_fit_loss_grad(pack, params, version, dt, radius, loss=loss, grad=grad)
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

        ops.mlapm_fit_loss_grad(pack, params, version, dt, radius, loss=loss, grad=grad)    # also sizes the workspace
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
        final, _ = ops.mlapm_fit_loss_grad(pack, params, version, dt, radius)
        out = params.double().cpu().tolist()
    res = {'version': version}
    res.update({k: float(val) for k, val in zip(PARAM_NAMES, out)})
    return CalibrationResult(params=res, initial_loss=float(initial.item()), final_loss=float(final.item()),
                             history=hist[:steps].cpu().tolist(), steps=steps, fit=tuple(fit))


def _parse_init(text):
    out = {}
    for item in filter(None, (s.strip() for s in (text or '').split(','))):
        k, _, val = item.partition('=')
        if k not in PARAM_NAMES or not _:
            raise argparse.ArgumentTypeError(f'--init expects name=value with names in {PARAM_NAMES}, got {item!r}')
        out[k] = float(val)
    return out


def _parse_fit(text):
    names = tuple(filter(None, (s.strip() for s in text.split(','))))
    bad = [k for k in names if k not in PARAM_NAMES]
    if bad or not names:
        raise argparse.ArgumentTypeError(f'--fit expects names from {PARAM_NAMES}, got {text!r}')
    return names


def get_args(argv=None):
    p = argparse.ArgumentParser(description="fit MLAPM's constants (tau, A, B, C, D, theta) to a clip on the GPU")
    p.add_argument('--data', type=str, required=True, help='a v2.2 clip (.npy), recorded or written by piml_amd.simulate')
    p.add_argument('--version', type=str, default='GC', choices=['raw', 'GC', 'UCY'])
    p.add_argument('--init', type=_parse_init, default={}, help='starting constants, e.g. A=7.55,B=-3 (default: main_mlapm.py\'s)')
    p.add_argument('--fit', type=_parse_fit, default=PARAM_NAMES, help='constants to fit, e.g. A,B,theta (default: all six)')
    p.add_argument('--frames', type=str, default=None, help='training frames a:b (default: all)')
    p.add_argument('--valid_frames', type=str, default=None, help='held-out frames c:d: their loss is reported before and after')
    p.add_argument('--steps', type=int, default=500)
    p.add_argument('--lr', type=float, default=0.02, help='Adam step size relative to each constant\'s magnitude')
    p.add_argument('--radius', type=float, default=0.3)
    p.add_argument('--skip_frames', type=int, default=25, help='desired speed = mean |v| over this many frames after the start')
    p.add_argument('--no_graph', action='store_true', help='eager iterations instead of a replayed graph')
    p.add_argument('--out', type=str, default='params.json')
    return p.parse_args(argv)


def main(argv=None):
    a = get_args(argv)
    from .data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(a.data)
    pack = pack_clip(raw, frames=a.frames, skip_frames=a.skip_frames)
    init = {**DEFAULT_INIT, **a.init}
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


if __name__ == '__main__':
    main(sys.argv[1:])
