"""Time piml_track_stats beside piml_flow_stats on the same inputs, and record the findings.

Timing: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity (crowds from the MLAPM law, which is
cheap to simulate; the statistics do not care what drove them) and the recorded GC and UCY clips, all with the default
options (128 lags).  Device time per call from events around `reps` back-to-back calls of ops_metrics.track_stats_frames (a
memset and two launches), alternated with the same number of calls of ops_metrics.flow_stats_frames with its defaults and
no box (the yardstick: the newest sibling on the same positions); end to end = trackstats.track_stats with its read-back
and the host histograms, from a host clock.  Frame pairs: `frame_pairs_visited` = sum over tracks and lags L <= n_lags of
max(last - first + 1 - L, 0), the (t, t + L) pairs the lag sweep looks at, from the track rows; `frame_pairs_nominal` =
S N T' n_lags, what a sweep of whole windows would look at.

Findings: persistence time, MSD exponent, mean acceleration and mean straightness of the recorded GC and UCY clips against
MLAPM runs of the same scenes (the GC scenario; the UCY clip's own scene, scenarios.clip_scenario).

    python tools/time_trackstats.py [--reps 20] [--out profiles/trackstats_time.json] [--summary profiles/trackstats_summary.md]"""
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
N_LAGS = 128


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(P, V, M, n_active, dt, reps, rounds=3):
    from piml_amd import ops_metrics, trackstats
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    track = lambda: ops_metrics.track_stats_frames(P, M, dt, 0.1, N_LAGS, 64.0, 0.25, 40, None, na)
    flow = lambda: ops_metrics.flow_stats_frames(P, V, M, 0.1, 0.1, 60, 6.0, (1.0, 0.0), 0.5, 5.0, None, None, 0.5, None, na)
    for _ in range(3):
        out = track()
        flow()
    torch.cuda.synchronize()
    t_ms, f_ms = [], []
    for _ in range(rounds):                   # the two alternate, so that a busy neighbour hits both
        t_ms.append(_events(track, reps))
        f_ms.append(_events(flow, reps))
    t = time.perf_counter()
    for _ in range(reps):
        trackstats.track_stats(P, M, dt=dt, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / reps
    first, last = out['trk_first'].cpu().numpy(), out['trk_last'].cpu().numpy()
    span = np.where(first >= 0, last - first + 1, 0).astype(np.int64).reshape(-1)
    lags = np.arange(1, N_LAGS + 1, dtype=np.int64)
    visited = int(np.maximum(span[:, None] - lags[None, :], 0).sum())
    S, T, N = M.shape
    dev_ms, yard_ms = float(np.median(t_ms)), float(np.median(f_ms))
    return dict(device_ms=round(dev_ms, 4), device_ms_rounds=[round(x, 4) for x in t_ms],
                flow_stats_device_ms=round(yard_ms, 4), flow_stats_device_ms_rounds=[round(x, 4) for x in f_ms],
                ratio_to_flow_stats=round(dev_ms / yard_ms, 3), end_to_end_ms=round(e2e_ms, 4),
                tracks=int((span > 0).sum()), mean_span_frames=round(float(span[span > 0].mean()), 1) if (span > 0).any() else 0,
                frame_pairs_visited=visited, frame_pairs_nominal=int(S) * int(T) * int(N) * N_LAGS,
                frame_pairs_per_s=float(f'{visited / (dev_ms * 1e-3):.4g}'))


def finding(st, min_count=50):
    rnd = lambda x: None if not np.isfinite(x) else round(float(x), 4)
    p = st.pooled()
    A, m, tau = st.heading_autocorrelation(min_count), st.msd(min_count), st.lag_times
    pick = [k for k in (0, 3, 7, 15, 31, 63, 127) if k < len(tau)]
    return dict(dt=st.options['dt'], persistence_time_s=rnd(st.persistence_time(min_count)),
                msd_exponent=rnd(st.msd_exponent(min_count)), mean_acceleration=rnd(st.mean_acceleration()),
                mean_straightness=rnd(st.mean_straightness()), mean_straightness_complete=rnd(st.mean_straightness('complete')),
                tracks=int(p.straight_n[0, 0]), complete_tracks=int(p.straight_n[0, 1]), acc_items=int(p.acc.sum()),
                acc_beyond_bins=int(p.acc[0, -1]), msd_far=int(p.msd_far.sum()),
                A={f'{tau[k]:.2f}': rnd(A[k]) for k in pick}, msd={f'{tau[k]:.2f}': rnd(m[k]) for k in pick})


def summary(res):
    rows = ['# Track statistics (`piml_track_stats`, DESIGN 4.22) on one MI355X', '',
            f'`python tools/time_trackstats.py --reps {res["reps"]}` (`trackstats_time.json`): GC ensembles driven by the MLAPM '
            f'law, 750 frames, capacity {res.get("capacity")}, and the recorded clips; default options, {N_LAGS} lags; device '
            'time per call = median of 3 rounds of events around back-to-back calls, alternated with `piml_flow_stats` '
            '(defaults, no box) on the same inputs (the yardstick).', '',
            '| input | track_stats device ms | flow_stats device ms | ratio | end to end ms | tracks | mean span | frame pairs '
            'visited | nominal S N T L | pairs / s |', '|---|---|---|---|---|---|---|---|---|---|']
    items = [(f'GC S = {S} x 750', r) for S, r in res['gc'].items()]
    items += [(f'recorded {k.upper()} clip', res[f'recorded_{k}_clip']) for k in CLIPS if f'recorded_{k}_clip' in res]
    for tag, r in items:
        rows.append(f'| {tag} | {r["device_ms"]} | {r["flow_stats_device_ms"]} | {r["ratio_to_flow_stats"]} | '
                    f'{r["end_to_end_ms"]} | {r["tracks"]} | {r["mean_span_frames"]} | {r["frame_pairs_visited"]:.4g} | '
                    f'{r["frame_pairs_nominal"]:.4g} | {r["frame_pairs_per_s"]:.3g} |')
    if 'findings' in res:
        rows += ['', 'Findings (`findings` in `trackstats_time.json`, `min_count` 50; recorded, not asserted):', '',
                 '| crowd | persistence time s | MSD exponent | mean acceleration m/s^2 | mean straightness (complete) | '
                 'tracks (complete) | A(tau) |', '|---|---|---|---|---|---|---|']
        for k, v in res['findings'].items():
            rows.append(f'| {k} | {v["persistence_time_s"]} | {v["msd_exponent"]} | {v["mean_acceleration"]} | '
                        f'{v["mean_straightness"]} ({v["mean_straightness_complete"]}) | {v["tracks"]} '
                        f'({v["complete_tracks"]}) | {v["A"]} |')
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
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS, clip_scenario
    from piml_amd.trackstats import track_stats_of_raw
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    res = {'frames': 750, 'reps': a.reps, 'n_lags': N_LAGS, 'gc': {}}
    gc8 = None
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        res['capacity'] = cap
        r = time_one(ens.position, ens.velocity, ens.mask_p, [min(int(n), cap) for n in ens.spawned], float(ens.time_unit),
                     a.reps)
        res['gc'][str(S)] = r
        print(f'[trackstats] GC S={S} x 750 frames, cap {cap}: {r}', flush=True)
        if S == 8 and a.findings:
            gc8 = ens.track_stats()
        del ens
    raws = {}
    dev = lambda x: x.to('cuda').contiguous()
    for k, path in CLIPS.items():
        raws[k] = RawData()
        raws[k].load_trajectory_data(os.path.join(ROOT, path))
        raw = raws[k]
        r = time_one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, float(raw.time_unit),
                     a.reps)
        res[f'recorded_{k}_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
        print(f'[trackstats] recorded {k} clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    if a.findings:
        f = {'recorded_gc_clip': finding(track_stats_of_raw(raws['gc'])),
             'recorded_ucy_clip': finding(track_stats_of_raw(raws['ucy']))}
        if gc8 is not None:
            f['mlapm_gc_ensemble_8x750'] = finding(gc8)
        ucy_scene = clip_scenario(raws['ucy']).to('cuda')
        ucy_law = MLAPM(version='UCY', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
        f[f'mlapm_ucy_clip_scene_8x{raws["ucy"].num_steps}'] = finding(
            ucy_law.simulate_ensemble(ucy_scene, raws['ucy'].num_steps, list(range(8))).track_stats())
        for k, v in f.items():
            print(f'[trackstats] {k}: {v}', flush=True)
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
