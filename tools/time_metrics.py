"""HIP-event timing of the evaluation metrics: impl='torch' (batched torch, functions/metrics.py) against impl='hip'
(the per-frame kernels of csrc/metrics.hip) on the GC test clip of tests/golden/rollout.npz (160 frames x 122 agents,
the pinnsf_m weights stored with it):
  eval_ms      BaseSimulator.test_multiple_rollouts on the clip (rollout + every metric), the two impls alternated
  metrics_ms   ot_with_time_mask + mmd_with_time_mask ('sum') on that evaluation's predictions alone
  kernel_ms    one launch of each kernel on the same frames, and on synthetic frames of 1024 and 4096 points (MMD's
               float64 exp rate = pairs x kernel_num / time)
Prints one JSON object.  Usage: python tools/time_metrics.py [--reps 10]
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_metrics.py --reps 2"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def timed(fn, reps):
    """median of `reps` HIP-event-timed calls (ms), each ending in a device synchronise"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    reps = ap.parse_args().reps
    from conftest import golden
    from test_simulator_gpu import load_data, make_sim, sim_args
    from piml_amd import ops_metrics
    from piml_amd.functions import metrics as M
    g = golden('rollout')
    res = {'reps': reps}
    sims = {impl: make_sim(g, sim_args(metrics_impl=impl), 'sd_m/') for impl in ('torch', 'hip')}
    d = load_data(g, 'roll')
    for impl, sim in sims.items():                                  # warm-up: code objects, graphs, allocator
        sim.test_multiple_rollouts([d], load_model=False)
    ev = {'torch': [], 'hip': []}
    for _ in range(reps):                                           # alternated: the host is shared
        for impl, sim in sims.items():
            ev[impl].append(timed(lambda: sim.test_multiple_rollouts([d], load_model=False), 1))
    res['eval_ms'] = {k: sorted(v)[len(v) // 2] for k, v in ev.items()}
    res['eval'] = {k: {m: s.last_eval[m] for m in ('ot', 'mmd')} for k, s in sims.items()}

    sim = sims['torch']
    with torch.no_grad():
        pred = sim.get_multiple_rollouts(d, t_start=sim.args.skip_frames, load_model=False)
        mask = d.mask_p_pred.long()
        p = sim.post_process(d, pred.position, pred.mask_p, mask)
    q = d.labels[..., :2]
    res['metrics_ms'] = {}
    for impl in ('torch', 'hip'):
        fn = lambda: (M.ot_with_time_mask(p, q, mask, reduction='sum', impl=impl),                  # noqa: E731
                      M.mmd_with_time_mask(p, q, mask, reduction='sum', impl=impl))
        fn()
        res['metrics_ms'][impl] = timed(fn, reps)
    x, y, m = M._selected_frames(p, q, mask)
    res['frames'] = int(x.shape[0])
    res['agents_per_frame_max'] = int(m.sum(-1).max())
    kernels = {'clip': (x, y, m)}
    gen = torch.Generator().manual_seed(0)
    for n, F in ((1024, 8), (4096, 1)):
        xs = 20 * torch.rand(F, n, 2, generator=gen)
        kernels[f'syn{n}x{F}'] = (xs.to('cuda'), (xs + 0.3 * torch.randn(F, n, 2, generator=gen)).to('cuda'), None)
    res['kernel_ms'] = {}
    for tag, (a, b, mm) in kernels.items():
        ops_metrics.sinkhorn_frames(a, b, mm, mm)
        ops_metrics.mmd_frames(a, b, mm, mm)
        it = ops_metrics.sinkhorn_frames(a, b, mm, mm)[1]
        t_ot = timed(lambda: ops_metrics.sinkhorn_frames(a, b, mm, mm), reps)
        t_mmd = timed(lambda: ops_metrics.mmd_frames(a, b, mm, mm), reps)
        cnt = (mm.sum(-1) if mm is not None else torch.full((a.shape[0],), a.shape[1], device=a.device)).double()
        pairs = float(((2 * cnt) * (2 * cnt - 1) / 2).sum())
        res['kernel_ms'][tag] = dict(frames=int(a.shape[0]), sinkhorn=t_ot, sinkhorn_iters_mean=float(it.float().mean()),
                                     mmd=t_mmd, mmd_f64_exp_per_s=pairs * 5 / (t_mmd * 1e-3))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
