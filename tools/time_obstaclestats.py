"""Time piml_obstacle_stats beside a plain torch restatement of its clearance histogram, and record the findings.

Timing: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity against the GC scene's 4094 obstacle
points (crowds from the MLAPM law, which is cheap to simulate and walks through the walls) and the recorded GC clip against
the same points, all with the default options.  Device time per call from events around `reps` back-to-back calls of
ops_metrics.obstacle_stats_frames (a memset and two launches), median of three rounds, alternated with the yardstick on the
same GPU: the clearance histogram alone (`clear`, one of the nine device outputs) in plain torch -- the participants of a
chunk of frames gathered, torch.cdist against the valid points, a row minimum, floor(r / r_bin) and a bincount -- which is
what a user without the kernel would write first.  End to end = obstaclestats.obstacle_stats with its read-back and the host
histograms, from a host clock.  Point evaluations = (focal agent-frames) x (valid points): each is a distance, a
point-to-segment distance and the time-to-obstacle test.

Findings: hit and contact figures of MLAPM GC ensembles against the recorded GC clip on the same obstacle points.

    python tools/time_obstaclestats.py [--reps 10] [--out profiles/obstaclestats_time.json]"""
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
VALU_LANE_OPS_PER_S = 78.6e12                 # 256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz (157.3 TFLOP/s of FMAs)


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_clearance_hist(P, V, M, n_active, obs, r_bin=0.05, r_bins=100, chunk_items=1 << 15):
    """`clear` (S, r_bins + 1) in plain torch: the participants gathered, cdist against the valid points in chunks of items, a
    row minimum, a bincount per member (distances as torch.cdist rounds them: not bit for bit the kernel's)."""
    S, T, N = M.shape
    pts = obs[torch.isfinite(obs).all(1)]
    slot = torch.arange(N, device=P.device)
    part = (M == 1) & (P.abs() < 65536).all(-1) & (V.abs() < 1024).all(-1)
    if n_active is not None:
        part &= slot[None, None, :] < n_active[:, None, None]
    s_idx = part.nonzero()[:, 0]
    p = P[part]
    bins = torch.empty(p.shape[0], device=P.device, dtype=torch.int64)
    for lo in range(0, p.shape[0], chunk_items):
        r = torch.cdist(p[lo:lo + chunk_items], pts).min(1).values
        bins[lo:lo + chunk_items] = torch.clamp(torch.floor(r / r_bin), max=r_bins).to(torch.int64)
    return torch.bincount(s_idx * (r_bins + 1) + bins, minlength=S * (r_bins + 1)).reshape(S, r_bins + 1)


def time_one(P, V, M, n_active, obs, dt, reps, rounds=3):
    from piml_amd import obstaclestats, ops_metrics
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    call = lambda: ops_metrics.obstacle_stats_frames(P, V, M, obs, dt, n_active=na)
    yard = lambda: torch_clearance_hist(P, V, M, na, obs)
    for _ in range(2):                        # warm-up of both at the timed shape
        out = call()
        mine = yard()
    torch.cuda.synchronize()
    k_ms, y_ms = [], []
    for _ in range(rounds):                   # the two alternate, so that a busy neighbour hits both
        k_ms.append(_events(call, reps))
        y_ms.append(_events(yard, max(reps // 4, 1)))
    t = time.perf_counter()
    for _ in range(max(reps // 2, 1)):
        obstaclestats.obstacle_stats(P, V, M, obs, dt=dt, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / max(reps // 2, 1)
    clear = out['clear'].cpu().numpy()
    n_valid = int(torch.isfinite(obs).all(1).sum())
    items = int(clear.sum())
    evals = items * n_valid
    dev_ms, yard_ms = float(np.median(k_ms)), float(np.median(y_ms))
    # the yardstick's distances round differently: its histogram may move an item across a bin edge
    moved = int(np.abs(clear - mine.cpu().numpy()).sum() // 2)
    return dict(device_ms=round(dev_ms, 4), device_ms_rounds=[round(x, 4) for x in k_ms],
                torch_clearance_ms=round(yard_ms, 4), torch_clearance_ms_rounds=[round(x, 4) for x in y_ms],
                torch_over_kernel=round(yard_ms / dev_ms, 3), end_to_end_ms=round(e2e_ms, 4), focal_items=items,
                valid_points=n_valid, point_evaluations=evals, point_evaluations_per_s=float(f'{evals / (dev_ms * 1e-3):.4g}'),
                items_binned_differently_by_torch=moved)


def finding(st):
    rnd = lambda x: None if not np.isfinite(x) else round(float(x), 5)
    p = st.pooled()
    sp = st.speed_by_clearance()
    return dict(focal=int(p.focal[0]), steps=int(p.steps[0]), contacts=int(p.contact[0]), hits=int(p.hit[0]),
                tracks=int(p.tracks[0]), tracks_hit=int(p.tracks_hit[0]), tracks_contact=int(p.tracks_contact[0]),
                contact_rate=rnd(st.contact_rate()), hit_rate=rnd(st.hit_rate()), hit_track_fraction=rnd(st.hit_track_fraction()),
                contact_track_fraction=rnd(st.contact_track_fraction()), mean_clearance=rnd(st.mean_clearance()),
                speed_by_clearance={f'{st.r_centres[k]:.3f}': rnd(sp[k]) for k in (2, 5, 10, 20, 40, 80) if k < len(sp) - 1})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--members', type=str, default='1,8,32')
    ap.add_argument('--no-findings', dest='findings', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import _lib
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.obstaclestats import compare_obstacle_stats, obstacle_stats_of_raw
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to('cuda')
    obs = sc.obstacles.contiguous()
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    usage = _lib.kernel_resource_usage()
    res = {'frames': 750, 'reps': a.reps, 'obstacle_points': int(obs.shape[0]), 'gc': {},
           'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                       for k, v in usage.items() if k.startswith('obstacle_stats')}}
    sims = {}
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        res['capacity'] = cap
        r = time_one(ens.position, ens.velocity, ens.mask_p, [min(int(n), cap) for n in ens.spawned], obs,
                     float(ens.time_unit), a.reps)
        res['gc'][str(S)] = r
        print(f'[obstaclestats] GC S={S} x 750 frames, cap {cap}: {r}', flush=True)
        if a.findings:
            sims[S] = ens.obstacle_stats()
        del ens
    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    dev = lambda x: x.to('cuda').contiguous()
    r = time_one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, obs, float(raw.time_unit),
                 a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    print(f'[obstaclestats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    best = res['gc'][max(res['gc'], key=int)]
    res['valu_lane_ops_per_s'] = VALU_LANE_OPS_PER_S
    res['evaluations_per_s_at_largest'] = best['point_evaluations_per_s']
    if a.findings:
        rec = obstacle_stats_of_raw(raw, obs)
        f = {'recorded_gc_clip': finding(rec)}
        for S, st in sims.items():
            f[f'mlapm_gc_ensemble_{S}x750'] = finding(st)
            f[f'mlapm_gc_ensemble_{S}x750_vs_recorded'] = {k: (None if isinstance(v, float) and not np.isfinite(v) else v)
                                                          for k, v in compare_obstacle_stats(st, rec).items()}
        for k, v in f.items():
            print(f'[obstaclestats] {k}: {v}', flush=True)
        res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
