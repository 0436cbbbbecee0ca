"""Time the group statistics and record the findings.

Three calls with the default options: the recorded GC clip, a GC ensemble of 32 members x 750 frames at the default capacity
(crowds from the MLAPM law, which is cheap to simulate) and one planted case of N = 4096 slots over T = 64 frames (a third
of the slots planted as pairs and triples, min_time scaled to the 64 frames).  Device time per call from events around
`reps` back-to-back calls, warmed, median of three rounds: pass 1 alone (ops_metrics.group_pairs_frames: three memsets and
one launch), pass 2 alone on the links of the case (ops_metrics.group_members_frames: five memsets and one launch), and the
whole operator ops_metrics.group_stats_frames, which reads the candidate counts back between the passes and sorts the rows
(a host clock around calls that end in a synchronise).  End to end = groupstats.group_stats with its read-back and the host
half.  Next to every time: the pair-frames pass 1 swept and the together pair-frames of the links pass 2 visited.

    python tools/time_groupstats.py [--reps 10] [--members 32] [--out profiles/groupstats_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _host(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def time_one(P, M, n_active, dt, reps, rounds=3, **kw):
    from piml_amd import groupstats, ops_metrics
    o = dict(groupstats.DEFAULTS, dt=dt)
    o.update(kw)
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    r2, dv2, vm2, min_frames, share_q = ops_metrics.group_thresholds(o['dt'], o['radius'], o['dv_max'], o['v_min'], o['min_time'],
                                                                     o['share'])
    full = lambda: ops_metrics.group_stats_frames(P, M, n_active=na, **o)
    out = full()
    link = out['edges'][:, 4] * 1024 >= share_q * out['edges'][:, 3]
    links = out['edges'][link][:, :3].to(torch.int32).contiguous()
    pass1 = lambda: ops_metrics.group_pairs_frames(P, M, r2, dv2, vm2, min_frames, None, na)
    pass2 = lambda: ops_metrics.group_members_frames(P, M, links, r2, dv2, vm2, o['r_bin'], o['r_bins'], o['a_bins'])
    for _ in range(2):                        # warm-up of all at the timed shape
        pass1(), pass2(), full()
    torch.cuda.synchronize()
    p1, p2, op = [], [], []
    for _ in range(rounds):
        p1.append(_events(pass1, reps))
        p2.append(_events(pass2, reps))
        op.append(_host(full, reps))
    e2e = _host(lambda: groupstats.group_stats(P, M, n_active=n_active, **o), max(reps // 2, 1))
    st = groupstats.group_stats(P, M, n_active=n_active, **o)
    pairs = int(st.pairs.sum())
    med = lambda x: float(np.median(x))
    return st, dict(pass1_ms=round(med(p1), 4), pass1_ms_rounds=[round(x, 4) for x in p1], pass2_ms=round(med(p2), 4),
                    pass2_ms_rounds=[round(x, 4) for x in p2], operator_ms=round(med(op), 4),
                    operator_ms_rounds=[round(x, 4) for x in op], end_to_end_ms=round(e2e, 4), pair_frames=pairs,
                    together=int(st.together.sum()), candidates=int(st.candidates.sum()), links=int(st.links.sum()),
                    link_frames=int(st.link_frames.sum()), pair_frames_per_s=float(f'{pairs / (med(p1) * 1e-3):.4g}'))


def finding(st):
    rnd = lambda a: [None if not np.isfinite(x) else round(float(x), 4) for x in np.asarray(a, np.float64).ravel()]
    p = st.pooled()
    return dict(eligible_tracks=st.eligible_tracks(), links=int(p.links[0]), size_tracks=p.size_tracks[0].tolist(),
                group_fraction=rnd(st.group_fraction())[0], speed_by_size=rnd(st.speed_by_size()), speed_ratio=rnd(st.speed_ratio())[0],
                mean_member_distance=rnd(st.mean_member_distance())[0], abreast_density=rnd(st.abreast_density()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    import groupstats_ref as REF
    from piml_amd import _lib
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    usage = _lib.kernel_resource_usage()
    res = {'reps': a.reps, 'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                                       for k, v in usage.items() if k.startswith('group_')}}
    f = {}
    dev = lambda x: torch.as_tensor(x).to('cuda').contiguous()
    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    st, r = time_one(dev(raw.position)[None], dev(raw.mask_p)[None], None, float(raw.time_unit), a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    f['recorded_gc_clip'] = finding(st)
    print(f'[groupstats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    P, M, _ = REF.planted_tracks(1, 64, 4096, seed=0)
    st, r = time_one(dev(P), dev(M), None, 0.08, a.reps, min_time=20.5 * 0.08)
    res['planted_4096x64'] = dict(frames=64, agents=4096, min_frames=21, **r)
    f['planted_4096x64'] = finding(st)
    print(f'[groupstats] planted N = 4096, T = 64: {r}', flush=True)
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    ens = law.simulate_ensemble(sc, 750, list(range(a.members)))
    cap = ens.position.shape[2]
    st, r = time_one(ens.position, ens.mask_p, [min(int(n), cap) for n in ens.spawned], float(ens.time_unit), a.reps)
    res['gc_ensemble'] = dict(members=a.members, frames=750, capacity=cap, **r)
    f[f'mlapm_gc_ensemble_{a.members}x750'] = finding(st)
    print(f'[groupstats] GC S={a.members} x 750 frames, cap {cap}: {r}', flush=True)
    for k, v in f.items():
        print(f'[groupstats] {k}: {v}', flush=True)
    res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
