"""Time piml_flow_stats against piml_pair_stats at lag 0 on the same inputs, and record the findings.

Timing: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity (crowds from the MLAPM law, which is
cheap to simulate; the statistics do not care what drove them) with the GC box, and the recorded GC clip, all with the
default options.  Device time per call from events around `reps` back-to-back calls of ops_metrics.flow_stats_frames (a
memset and two launches), alternated with the same number of calls of ops_metrics.pair_stats_frames with no lags and
r_max = 6 m (the yardstick: the same focal agents, the same sources, the same cut-off); end to end = flowstats.flow_stats
with its read-back, from a host clock.  Pair evaluations: the yardstick's own `pairs` count (ordered pairs of a focal
agent and a participant within r_max), the pairs the flow sweep visits within r_max too; the flow sweep also visits every
pair beyond r_max once, like the yardstick, so `pairs_swept` = sum over slices of focal x (participants - 1) is given too.

Findings: C(r), the correlation length, the lane order and the same-direction fraction against chance of the recorded GC
(GC box) and UCY clips and of an MLAPM crosswalk ensemble.

    python tools/time_flowstats.py [--reps 20] [--out profiles/flowstats_time.json] [--summary profiles/flowstats_summary.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CLIPS = {'gc': 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy',
         'ucy': 'tests/golden/data/UCY_Dataset_time162-216_timeunit0.08.npy'}
BOX = (5.0, 25.0, 15.0, 35.0)
R_MAX = 6.0


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(P, V, M, n_active, box, reps, rounds=3):
    from piml_amd import flowstats, ops_metrics
    from piml_amd.crowdstats import grid_shape
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    flow = lambda: ops_metrics.flow_stats_frames(P, V, M, 0.1, 0.1, 60, R_MAX, (1.0, 0.0), 0.5, 5.0, box,
                                                 grid_shape(box, 0.5), 0.5, None, na)
    pair = lambda: ops_metrics.pair_stats_frames(P, V, M, 0.5, (), 0.1, 100, 0.05, 100, R_MAX, box, None, na)
    for _ in range(3):
        flow()
        ref = pair()
    torch.cuda.synchronize()
    f_ms, p_ms = [], []
    for _ in range(rounds):                   # the two alternate, so that a busy neighbour hits both
        f_ms.append(_events(flow, reps))
        p_ms.append(_events(pair, reps))
    t = time.perf_counter()
    for _ in range(reps):
        flowstats.flow_stats(P, V, M, box=box, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / reps
    part = (M == 1) & torch.isfinite(P).all(-1) & torch.isfinite(V).all(-1)
    if na is not None:
        part &= torch.arange(M.shape[2], device=M.device)[None, None, :] < na[:, None, None]
    focal = part & (P[..., 0] >= box[0]) & (P[..., 0] < box[1]) & (P[..., 1] >= box[2]) & (P[..., 1] < box[3])
    swept = int((focal.sum(-1) * (part.sum(-1) - 1).clamp(min=0)).sum().item())
    pairs = int(ref['pairs'].sum().item())
    dev_ms, yard_ms = float(np.median(f_ms)), float(np.median(p_ms))
    return dict(device_ms=round(dev_ms, 4), device_ms_rounds=[round(x, 4) for x in f_ms],
                pair_stats_lag0_device_ms=round(yard_ms, 4), pair_stats_lag0_device_ms_rounds=[round(x, 4) for x in p_ms],
                ratio_to_pair_stats=round(dev_ms / yard_ms, 3), end_to_end_ms=round(e2e_ms, 4),
                pair_evaluations_within_r_max=pairs, pairs_swept=swept,
                pair_evaluations_per_s=float(f'{pairs / (dev_ms * 1e-3):.4g}'),
                pairs_swept_per_s=float(f'{swept / (dev_ms * 1e-3):.4g}'))


def finding(st, min_count=50):
    c, r = st.velocity_correlation(min_count), st.r_centres
    ok = np.nonzero(np.isfinite(c))[0]
    same, chance = st.same_direction_fraction(), st.chance_same_fraction()
    rnd = lambda x: None if not np.isfinite(x) else round(float(x), 4)
    p = st.pooled()
    return dict(axis=[round(v, 6) for v in st.options['axis']], correlation_length_m=rnd(st.correlation_length(min_count)),
                lane_order=rnd(st.lane_order()[1]), lane_agent_frames=int(p.lane_n.sum()),
                same_direction_fraction=rnd(same), chance_same_fraction=rnd(chance), excess_same_fraction=rnd(same - chance),
                dir_plus=int(p.dir_plus.sum()), dir_minus=int(p.dir_minus.sum()), corr_pairs=int(p.corr_pairs.sum()),
                C={f'{r[k]:.2f}': round(float(c[k]), 4) for k in ok[::5]})


def summary(res):
    rows = ['# Collective-motion statistics (`piml_flow_stats`, DESIGN 4.21) on one MI355X', '',
            f'`python tools/time_flowstats.py --reps {res["reps"]}` (`flowstats_time.json`): GC ensembles driven by the MLAPM '
            f'law, 750 frames, capacity {res.get("capacity")}, GC box, default options; device time per call = median of 3 '
            'rounds of events around back-to-back calls, alternated with `piml_pair_stats` without lags at `r_max` 6 m on '
            'the same inputs (the yardstick).', '',
            '| input | flow_stats device ms | pair_stats lag 0 device ms | ratio | end to end ms | pairs within r_max / s | '
            'pairs swept / s |', '|---|---|---|---|---|---|---|']
    items = [(f'GC S = {S} x 750', r) for S, r in res['gc'].items()] + [('recorded GC clip', res['recorded_gc_clip'])]
    for tag, r in items:
        rows.append(f'| {tag} | {r["device_ms"]} | {r["pair_stats_lag0_device_ms"]} | {r["ratio_to_pair_stats"]} | '
                    f'{r["end_to_end_ms"]} | {r["pair_evaluations_per_s"]:.3g} | {r["pairs_swept_per_s"]:.3g} |')
    if 'findings' in res:
        rows += ['', 'Findings (`findings` in `flowstats_time.json`, `min_count` 50):', '',
                 '| crowd | axis | correlation length m | lane order | same-direction fraction | chance | C(r) |',
                 '|---|---|---|---|---|---|---|']
        for k, v in res['findings'].items():
            rows.append(f'| {k} | {v["axis"]} | {v["correlation_length_m"]} | {v["lane_order"]} | '
                        f'{v["same_direction_fraction"]} | {v["chance_same_fraction"]} | {v["C"]} |')
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--members', type=str, default='1,8,32')
    ap.add_argument('--no-findings', dest='findings', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--summary', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd.data.data import RawData
    from piml_amd.flowstats import flow_stats_of_raw
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    res = {'frames': 750, 'reps': a.reps, 'r_max': R_MAX, 'r_bins': 60, 'box': list(BOX), 'gc': {}}
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        res['capacity'] = cap
        r = time_one(ens.position, ens.velocity, ens.mask_p, [min(int(n), cap) for n in ens.spawned], BOX, a.reps)
        res['gc'][str(S)] = r
        print(f'[flowstats] GC S={S} x 750 frames, cap {cap}: {r}', flush=True)
        del ens
    raws = {}
    for k, path in CLIPS.items():
        raws[k] = RawData()
        raws[k].load_trajectory_data(os.path.join(ROOT, path))
    raw = raws['gc']
    dev = lambda x: x.to('cuda').contiguous()
    r = time_one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, BOX, a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    print(f'[flowstats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    if a.findings:
        f = {}
        f['recorded_gc_clip_box_axis_auto'] = finding(flow_stats_of_raw(raws['gc'], box=BOX, axis='auto'))
        f['recorded_gc_clip_box_axis_x'] = finding(flow_stats_of_raw(raws['gc'], box=BOX))
        f['recorded_ucy_clip_axis_auto'] = finding(flow_stats_of_raw(raws['ucy'], axis='auto'))
        cw = SCENARIOS['crosswalk']().to('cuda')
        f['mlapm_crosswalk_ensemble_8x750_axis_auto'] = finding(
            law.simulate_ensemble(cw, 750, list(range(8))).flow_stats(axis='auto'))
        for k, v in f.items():
            print(f'[flowstats] {k}: {v}', flush=True)
        res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
