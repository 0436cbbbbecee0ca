"""Times of the MLAPM rollout calibration (piml_mlapm_rollout_fit_loss_grad, calibrate_mlapm(horizon=H)), one JSON object
on stdout:
  gc_h{8,16,32}_us     one loss + gradient evaluation on every window of the whole GC test clip at stride 1 (small form);
  ens4_h16_us          the same on the clips of a 4-member simulated GC ensemble packed as one (windows of > 64 agents in
                       the big form), with the window counts of each form;
  torch_gc_h16_us      the GC clip at H = 16 as batched float32 torch autograd over windows padded to the largest one;
  fit_iter_ms          one captured fit iteration (kernel + device Adam) on the GC clip at H = 16;
  one_step_vs_rollout  the held-out (500:700) H = 16 rollout loss and RMSE at k = 16 after a one-step fit and after a
                       rollout fit on frames 0:500, both from main_mlapm.py's constants (reported, not asserted anywhere).
Each time is the median of --reps timed runs of --inner back-to-back calls, after a warm-up.
Usage: python tools/time_mlapm_rollout_fit.py [--reps 7] [--inner 20] [--out profiles/mlapm_rollout_fit_time.json]"""
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
MAIN_MLAPM = dict(zip(('tau', 'A', 'B', 'C', 'D', 'theta'), INIT))


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


def torch_windows(pack, dev):
    """Batched float32 autograd of the GC rollout loss over a pack's windows padded to the largest one."""
    H = pack.horizon
    cnt = pack.slot_count
    W, n = len(cnt), max(cnt)
    R = torch.zeros(W, H + 1, n, 4)
    Dd = torch.zeros(W, H + 1, n, 2)
    Fl = torch.zeros(W, H + 1, n, dtype=torch.uint8)
    v0 = torch.zeros(W, n)
    off = pack.slot_offsets.cpu().tolist()
    rec, dst, flg, spd = pack.rec.cpu(), pack.destination.cpu(), pack.flags.cpu(), pack.desired_speed.cpu()
    for w in range(W):
        a, m = (H + 1) * off[w], cnt[w]
        R[w, :, :m] = rec[a:a + (H + 1) * m].reshape(H + 1, m, 4)
        Dd[w, :, :m] = dst[a:a + (H + 1) * m].reshape(H + 1, m, 2)
        Fl[w, :, :m] = flg[a:a + (H + 1) * m].reshape(H + 1, m)
        v0[w, :m] = spd[off[w]:off[w + 1]]
    R, Dd, v0 = R.to(dev), Dd.to(dev), v0.to(dev)
    pres, carr = (Fl & 1).bool().to(dev), (Fl & 4).bool().to(dev)
    prm = torch.tensor(INIT, device=dev, requires_grad=True)
    dt = pack.time_unit
    eye = torch.eye(n, dtype=torch.bool, device=dev)

    def run():
        tau, A, B, C, D, th = prm
        p, v = R[:, 0, :, :2], R[:, 0, :, 2:]
        num, cnt_ = 0.0, 0
        for k in range(H):
            ok = pres[:, k]
            ed = torch.nn.functional.normalize(Dd[:, k] - p, dim=-1)
            force = (v0[..., None] * ed - v) / tau
            vr = p[:, None, :, :] - p[:, :, None, :]
            vv = v[:, None, :, :] - v[:, :, None, :]
            r = vr.norm(dim=-1)
            view = (torch.einsum('wnk,wnmk->wnm', v, vr) > 0) & ok[:, None, :] & ~eye
            cos = torch.nn.functional.cosine_similarity(vr, vv, dim=-1)
            sg = -(vr[..., 0] * ed[:, :, None, 1] - vr[..., 1] * ed[:, :, None, 0]).sign()
            sg = torch.where(sg == 0, torch.ones_like(sg), sg)
            ang = sg * th / 180 * math.pi
            n_ = torch.nn.functional.normalize(vr, dim=-1)
            c, s = ang.cos(), ang.sin()
            dx, dy = c * n_[..., 0] - s * n_[..., 1], s * n_[..., 0] + c * n_[..., 1]
            g = view * A * torch.exp(B * r + C * cos + D * r * cos)
            force = force - torch.stack(((g * dx).sum(-1), (g * dy).sum(-1)), -1)
            vn = v + force * dt
            pn = p + vn * dt
            cr = carr[:, k + 1, :, None]
            p = torch.where(cr, pn, R[:, k + 1, :, :2])
            v = torch.where(cr, vn, R[:, k + 1, :, 2:])
            num = num + (((p - R[:, k + 1, :, :2]) ** 2).sum(-1) * carr[:, k + 1]).sum()
            cnt_ += carr[:, k + 1].sum()
        loss = num / cnt_
        return torch.autograd.grad(loss, prm)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--fit_steps', type=int, default=200)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    from piml_amd import ops
    from piml_amd.calibrate import calibrate_mlapm, mlapm_rollout_fit_loss, pack_windows
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import gc_scenario
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0)}
    raw = RawData()
    raw.load_trajectory_data(GC_CLIP)
    prm = torch.tensor(INIT, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    grad = torch.empty(6, device=dev)
    for H in (8, 16, 32):
        pk = pack_windows(raw, H, device=dev)
        t = 1e3 * per_call_ms(lambda: ops.mlapm_rollout_fit_loss_grad(pk, prm, 'GC', 0.08, 0.3, 1.0, loss, grad),
                              a.reps, a.inner)
        res[f'gc_h{H}'] = {'windows': pk.num_windows, 'small': int(pk.small_windows.numel()), 'slots': pk.num_slots,
                           'terms': pk.num_terms, 'max_slots': max(pk.slot_count)}
        res[f'gc_h{H}_us'] = t
    pk16 = pack_windows(raw, 16, device=dev)
    res['torch_gc_h16_us'] = 1e3 * per_call_ms(torch_windows(pk16, dev), 3, 1)
    ens = MLAPM(version='GC', **MAIN_MLAPM).simulate_ensemble(gc_scenario().to(dev), 400, [0, 1, 2, 3])
    members = [ens.member(m) for m in range(4)]
    clips = [m.to_raw_data() for m in members]
    speeds = [m.desired_speed[:m.num_agents] for m in members]
    pe = pack_windows(clips, 16, frames='100:400', desired_speed=speeds, device=dev)
    res['ens4_h16'] = {'windows': pe.num_windows, 'small': int(pe.small_windows.numel()),
                       'big': int(pe.big_windows.numel()), 'slots': pe.num_slots, 'terms': pe.num_terms,
                       'max_slots': max(pe.slot_count)}
    res['ens4_h16_us'] = 1e3 * per_call_ms(lambda: ops.mlapm_rollout_fit_loss_grad(pe, prm, 'GC', 0.08, 0.3, 1.0, loss, grad),
                                           a.reps, max(1, a.inner // 4))

    def fit(steps):
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        calibrate_mlapm(pk16, version='GC', steps=steps, graph_steps=50, horizon=16)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    fit(a.fit_steps)
    d = [fit(a.fit_steps + 1) - fit(a.fit_steps // 2 + 1) for _ in range(3)]
    res['fit_iter_ms'] = statistics.median(d) / (a.fit_steps - a.fit_steps // 2)
    # held-out H = 16 error after a one-step fit and after a rollout fit (reported only)
    valid = pack_windows(raw, 16, frames='500:700', device=dev)
    out = {}
    for name, kw in (('main_mlapm', None), ('one_step', {}), ('rollout_h16', {'horizon': 16})):
        params = MAIN_MLAPM if kw is None else calibrate_mlapm(raw, version='GC', init=MAIN_MLAPM, frames='0:500',
                                                               steps=500, **kw).params
        lv, _, (sse, cnt) = mlapm_rollout_fit_loss(valid, params, 'GC', per_step=True)
        out[name] = {'heldout_loss_m2': lv, 'rmse_k16_m': math.sqrt(sse[-1] / cnt[-1]),
                     'params': {k: params[k] for k in MAIN_MLAPM}}
    res['one_step_vs_rollout'] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
