"""Time piml_line_stats beside a plain torch restatement of its `cross` and `nt` rows, and record the findings.

Timing: a GC ensemble of 32 members x 750 frames at the default capacity (crowds from the MLAPM law, which is cheap to
simulate) across three gate lines 2 m inside the hall's bottom, left and right entries, and the recorded GC clip across the
two mid-lines of its bounding box, all with the default options.  Device time per call from events around `reps`
back-to-back calls of ops_metrics.line_stats_frames (a memset and two launches), median of three rounds, alternated with the
yardstick on the same GPU: the `cross` and `nt` rows alone in plain torch -- the sides of every position against every line,
the two sign tests, the crossing point and 0 <= w < 1 on whole (S, T - 1, N) tensors, a sum over the slots -- which is what a
user without the kernel would write.  End to end = linestats.line_stats with its read-back and the host half, from a host
clock.  Items = steps x lines.

Findings: flows, mean crossing speeds and origin-destination counts of the ensemble and the clip.

    python tools/time_linestats.py [--reps 10] [--members 32] [--out profiles/linestats_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
GC_GATES = '0,2,30,2;2,5,2,17;28,7,28,26'


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_cross_nt(P, M, n_active, lines):
    """`nt` (S, L, 2, T) and `cross` (S, L, 2) in plain torch (its products may contract: not bit for bit the kernel's)."""
    S, T, N = M.shape
    part = (M == 1) & (P.abs() < 65536).all(-1)
    if n_active is not None:
        part &= torch.arange(N, device=P.device)[None, None, :] < n_active[:, None, None]
    ex = part[:, :-1] & part[:, 1:]
    Pz = torch.where(part[..., None], P, torch.zeros_like(P))
    p0, p1 = Pz[:, :-1], Pz[:, 1:]
    nt = torch.zeros(S, lines.shape[0], 2, T, device=P.device, dtype=torch.int64)
    for l in range(lines.shape[0]):
        ax, ay, bx, by = lines[l]
        dx, dy = bx - ax, by - ay
        s0 = dx * (p0[..., 1] - ay) - dy * (p0[..., 0] - ax)
        s1 = dx * (p1[..., 1] - ay) - dy * (p1[..., 0] - ax)
        fwd, back = ex & (s0 < 0) & (s1 >= 0), ex & (s0 >= 0) & (s1 < 0)
        f = s0 / torch.where(fwd | back, s0 - s1, torch.ones_like(s0))
        cx, cy = p0[..., 0] + f * (p1[..., 0] - p0[..., 0]), p0[..., 1] + f * (p1[..., 1] - p0[..., 1])
        w = ((cx - ax) * dx + (cy - ay) * dy) / (dx * dx + dy * dy)
        inside = (w >= 0) & (w < 1)
        nt[:, l, 0, :-1] = (fwd & inside).sum(-1)
        nt[:, l, 1, :-1] = (back & inside).sum(-1)
    return nt.sum(-1), nt


def time_one(P, M, n_active, lines, dt, reps, rounds=3):
    from piml_amd import linestats, ops_metrics
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    lt = torch.from_numpy(linestats.check_lines(lines)).to(P.device)
    call = lambda: ops_metrics.line_stats_frames(P, M, lt, dt, n_active=na)
    yard = lambda: torch_cross_nt(P, M, na, lt)
    for _ in range(2):                        # warm-up of both at the timed shape
        out = call()
        mine = yard()
    torch.cuda.synchronize()
    k_ms, y_ms = [], []
    for _ in range(rounds):                   # the two alternate, so that a busy neighbour hits both
        k_ms.append(_events(call, reps))
        y_ms.append(_events(yard, max(reps // 2, 1)))
    t = time.perf_counter()
    for _ in range(max(reps // 2, 1)):
        linestats.line_stats(P, M, lines, dt=dt, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / max(reps // 2, 1)
    steps, cross = int(out['steps'].sum()), int(out['cross'].sum())
    items = steps * int(lt.shape[0])
    dev_ms, yard_ms = float(np.median(k_ms)), float(np.median(y_ms))
    moved = int((out['nt'] - mine[1]).abs().sum())      # the yardstick rounds differently: a crossing may move
    return dict(device_ms=round(dev_ms, 4), device_ms_rounds=[round(x, 4) for x in k_ms],
                torch_cross_nt_ms=round(yard_ms, 4), torch_cross_nt_ms_rounds=[round(x, 4) for x in y_ms],
                torch_over_kernel=round(yard_ms / dev_ms, 3), end_to_end_ms=round(e2e_ms, 4), lines=int(lt.shape[0]), steps=steps,
                crossings=cross, items=items, items_per_s=float(f'{items / (dev_ms * 1e-3):.4g}'),
                nt_entries_counted_differently_by_torch=moved)


def finding(st):
    rnd = lambda a: [None if not np.isfinite(x) else round(float(x), 4) for x in np.asarray(a, np.float64).ravel()]
    p = st.pooled()
    return dict(lines=st.lines.astype(np.float64).tolist(), cross=p.cross[0].tolist(), flow_per_s=rnd(st.flow()),
                specific_flow_per_s_m=rnd(st.specific_flow()), mean_crossing_speed=rnd(st.mean_crossing_speed()),
                mean_headway_s=rnd(st.mean_headway()), od_counts=st.od_counts().tolist(),
                mean_travel_time_s=rnd(st.mean_travel_time()), steps=int(p.steps[0]), tracks=int(p.tracks[0]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import _lib
    from piml_amd.crowdstats import auto_box
    from piml_amd.data.data import RawData
    from piml_amd.linestats import auto_lines, line_stats_of_raw, parse_lines
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    usage = _lib.kernel_resource_usage()
    res = {'frames': 750, 'reps': a.reps,
           'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                       for k, v in usage.items() if k.startswith('line_stats')}}
    gates = parse_lines(GC_GATES)
    ens = law.simulate_ensemble(sc, 750, list(range(a.members)))
    cap = ens.position.shape[2]
    r = time_one(ens.position, ens.mask_p, [min(int(n), cap) for n in ens.spawned], gates, float(ens.time_unit), a.reps)
    res['gc_ensemble'] = dict(members=a.members, capacity=cap, **r)
    print(f'[linestats] GC S={a.members} x 750 frames, cap {cap}: {r}', flush=True)
    f = {f'mlapm_gc_ensemble_{a.members}x750': finding(ens.line_stats(gates))}
    del ens
    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    mid = auto_lines(auto_box(raw.position.numpy(), raw.mask_p.numpy(), 0.5))
    dev = lambda x: x.to('cuda').contiguous()
    r = time_one(dev(raw.position)[None], dev(raw.mask_p)[None], None, mid, float(raw.time_unit), a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    print(f'[linestats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    f['recorded_gc_clip'] = finding(line_stats_of_raw(raw, mid))
    for k, v in f.items():
        print(f'[linestats] {k}: {v}', flush=True)
    res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
