"""Times of the MLAPM calibration (piml_mlapm_fit_loss_grad, piml_amd.calibrate), one JSON object on stdout:
  gc_clip_us          one loss + gradient evaluation on the whole GC test clip (750 frames, ~21 agents each, lane kernel);
  synth4096_us        the same on --frames synthetic frames of 4096 agents (wave kernel), and per ordered pair;
  fwd4096_pair_ns     mlapm_fwd_kernel (ops.mlapm_step, one 4096-agent frame) per ordered pair, for comparison;
  fit_iter_ms         one captured fit iteration (kernel + device Adam) on the GC clip, from the replay of K iterations;
  torch_*             the same loss + gradient as batched torch autograd over frames padded to the largest one (baseline).
Each figure is the median of --reps timed runs of --inner back-to-back calls, after a warm-up.
Usage: python tools/time_mlapm_fit.py [--reps 7] [--inner 50] [--frames 8] [--out profiles/mlapm_fit_time.json]"""
import argparse
import json
import math
import os
import statistics
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

GC_CLIP = os.path.join(ROOT, 'tests', 'golden', 'data', 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy')
INIT = [0.5, 7.55, -3.0, 0.2, -0.3, 56.0]


def per_call_ms(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out)


def torch_padded(pack, dev):
    """(F, n, .) padded frames of a pack and a batched-autograd GC loss over them (float32, the reference's expressions)."""
    off = pack.offsets.cpu().tolist()
    F = len(off) - 1
    n = max(b - a for a, b in zip(off[:-1], off[1:]))
    st = torch.zeros(F, n, 4, device=dev)
    de = torch.zeros(F, n, 2, device=dev)
    v0 = torch.zeros(F, n, device=dev)
    tg = torch.zeros(F, n, 2, device=dev)
    ok = torch.zeros(F, n, dtype=torch.bool, device=dev)
    foc = torch.zeros(F, n, dtype=torch.bool, device=dev)
    for f in range(F):
        a, b = off[f], off[f + 1]
        st[f, :b - a], de[f, :b - a], v0[f, :b - a] = pack.state[a:b], pack.destination[a:b], pack.desired_speed[a:b]
        t = pack.target[a:b]
        fin = torch.isfinite(t).all(-1)
        tg[f, :b - a] = torch.nan_to_num(t)
        ok[f, :b - a], foc[f, :b - a] = True, fin
    prm = torch.tensor(INIT, device=dev, requires_grad=True)
    dt = pack.time_unit

    def run():
        tau, A, B, C, D, th = prm
        p, v = st[..., :2], st[..., 2:]
        ed = torch.nn.functional.normalize(de - p, dim=-1)
        force = (v0[..., None] * ed - v) / tau
        vr = p[:, None, :, :] - p[:, :, None, :]
        vv = v[:, None, :, :] - v[:, :, None, :]
        r = vr.norm(dim=-1)
        view = (torch.einsum('fnk,fnmk->fnm', v, vr) > 0) & ok[:, None, :]
        cos = torch.nn.functional.cosine_similarity(vr, vv, dim=-1)
        sg = -(vr[..., 0] * ed[:, :, None, 1] - vr[..., 1] * ed[:, :, None, 0]).sign()
        sg = torch.where(sg == 0, torch.ones_like(sg), sg)
        ang = sg * th / 180 * math.pi
        n_ = torch.nn.functional.normalize(vr, dim=-1)
        c, s = ang.cos(), ang.sin()
        dx, dy = c * n_[..., 0] - s * n_[..., 1], s * n_[..., 0] + c * n_[..., 1]
        g = view * A * torch.exp(B * r + C * cos + D * r * cos)
        force = force - torch.stack(((g * dx).sum(-1), (g * dy).sum(-1)), -1)
        pred = v + force * dt
        loss = (((pred - tg) ** 2).sum(-1) * foc).sum() / foc.sum()
        return torch.autograd.grad(loss, prm)
    return run


def synth_raw(frames, N, seed=0):
    from piml_amd.data.data import RawData
    g = torch.Generator().manual_seed(seed)
    side = math.sqrt(N / 1.0)                          # ~1 agent per square metre
    p = torch.rand(frames + 1, N, 2, generator=g) * side
    v = torch.randn(frames + 1, N, 2, generator=g) * 0.5 + torch.tensor([1.0, 0.0])
    d = p[:1].expand(frames + 1, N, 2) + torch.tensor([side, 0.0])
    return RawData(position=p, velocity=v, destination=d.clone(), meta_data={'time_unit': 0.08})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--fit_steps', type=int, default=200)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, pack_clip
    from piml_amd.data.data import RawData
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0)}
    raw = RawData()
    raw.load_trajectory_data(GC_CLIP)
    pack = pack_clip(raw, device=dev)
    prm = torch.tensor(INIT, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    grad = torch.empty(6, device=dev)
    pairs = sum((b - a) * (b - a - 1) for a, b in zip(pack.offsets.cpu().tolist()[:-1], pack.offsets.cpu().tolist()[1:]))
    res['gc_clip'] = {'frames': len(pack.frames), 'entries': pack.num_entries, 'focal': pack.num_focal, 'ordered_pairs': pairs}
    res['gc_clip_us'] = 1e3 * per_call_ms(lambda: ops.mlapm_fit_loss_grad(pack, prm, 'GC', 0.08, 0.3, loss, grad), a.reps, a.inner)
    run = torch_padded(pack, dev)
    res['torch_gc_clip_us'] = 1e3 * per_call_ms(run, a.reps, max(1, a.inner // 10))
    # captured fit iterations: the time of `steps` iterations minus that of `steps / 2`, over the difference
    def fit(steps):
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        calibrate_mlapm(pack, version='GC', steps=steps, graph_steps=50)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    fit(a.fit_steps)
    d = [fit(a.fit_steps + 1) - fit(a.fit_steps // 2 + 1) for _ in range(3)]
    res['fit_iter_ms'] = statistics.median(d) / (a.fit_steps - a.fit_steps // 2)
    for N in (4096,):
        sp = pack_clip(synth_raw(a.frames, N), frames=range(a.frames), device=dev)
        t = 1e3 * per_call_ms(lambda: ops.mlapm_fit_loss_grad(sp, prm, 'GC', 0.08, 0.3, loss, grad), a.reps, max(1, a.inner // 5))
        res[f'synth{N}_us'] = t
        res[f'synth{N}_pair_ns'] = 1e3 * t / (a.frames * N * (N - 1))
        p, v = sp.state[:N, :2].contiguous(), sp.state[:N, 2:].contiguous()
        dd, s = sp.destination[:N].contiguous(), sp.desired_speed[:N].contiguous()
        kw = dict(zip(('tau', 'A', 'B', 'C', 'D', 'theta'), INIT))
        tf = 1e3 * per_call_ms(lambda: ops.mlapm_step(p, v, s, dd, 0.08, 0.3, version='GC', **kw), a.reps, a.inner)
        res[f'fwd{N}_us'] = tf
        res[f'fwd{N}_pair_ns'] = 1e3 * tf / (N * N)
        if a.frames * N * N * 4 * 20 < 4e10:                 # (the padded pair tensors of the batched baseline)
            run = torch_padded(sp, dev)
            res[f'torch_synth{N}_us'] = 1e3 * per_call_ms(run, 3, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
