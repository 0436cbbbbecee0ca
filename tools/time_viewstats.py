"""Time piml_view_stats against piml_pair_stats on the same inputs, and record the findings.

Timing: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity (crowds from the MLAPM law, which is
cheap to simulate; the statistics do not care what drove them) with the GC box, and the recorded GC clip, all with the
default options and the default lags (64, 128, 192).  Device time per call from events around `reps` back-to-back calls of
ops_metrics.view_stats_frames (a memset and two launches), alternated with the same number of calls of
ops_metrics.pair_stats_frames with its defaults, the same lags and the same box (the yardstick: the same pair slices, the
same sweep, less per pair); end to end = viewstats.view_stats with its read-back, from a host clock.  Pair evaluations:
the kernel's own `pairs` count over all lags.

Findings: front/back ratio, passing side against chance, mean front gap and headway fit of the recorded GC (GC box) and
UCY clips and of a 32-seed GC ensemble under the default GC law.

Identifiability: a reference ensemble simulated with theta = 56 (seeds 100..131) and candidates theta in {0, 28, 56, 84} on
seeds 0..15, which the reference did not use: calibrate.stats_objective of (crowd, pairs) and of (crowd, pairs, views).

    python tools/time_viewstats.py [--reps 20] [--out profiles/viewstats_time.json] [--summary profiles/viewstats_summary.md]"""
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
LAGS = (64, 128, 192)
LAW = dict(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
THETAS = (0.0, 28.0, 56.0, 84.0)


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(P, V, M, n_active, box, reps, rounds=3):
    from piml_amd import ops_metrics, viewstats
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    view = lambda: ops_metrics.view_stats_frames(P, V, M, LAGS, box=box, n_active=na)       # noqa: E731
    pair = lambda: ops_metrics.pair_stats_frames(P, V, M, lags=LAGS, box=box, n_active=na)  # noqa: E731
    for _ in range(3):
        got = view()
        ref = pair()
    torch.cuda.synchronize()
    v_ms, p_ms = [], []
    for _ in range(rounds):                   # the two alternate, so that a busy neighbour hits both
        v_ms.append(_events(view, reps))
        p_ms.append(_events(pair, reps))
    t = time.perf_counter()
    for _ in range(reps):
        viewstats.view_stats(P, V, M, box=box, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / reps
    pairs, yard_pairs = int(got['pairs'].sum().item()), int(ref['pairs'].sum().item())
    dev_ms, yard_ms = float(np.median(v_ms)), float(np.median(p_ms))
    return dict(device_ms=round(dev_ms, 4), device_ms_rounds=[round(x, 4) for x in v_ms],
                pair_stats_device_ms=round(yard_ms, 4), pair_stats_device_ms_rounds=[round(x, 4) for x in p_ms],
                ratio_to_pair_stats=round(dev_ms / yard_ms, 3), end_to_end_ms=round(e2e_ms, 4),
                pair_evaluations=pairs, pair_stats_pair_evaluations=yard_pairs,
                pair_evaluations_per_s=float(f'{pairs / (dev_ms * 1e-3):.4g}'))


def finding(st):
    rnd = lambda x: None if not np.isfinite(x) else round(float(x), 4)      # noqa: E731
    side, chance = st.passing_side()
    m, s = st.headway_fit()
    p = st.pooled()
    return dict(focal=int(p.focal[0, 0]), pairs=p.pairs[0].tolist(), front_back_ratio=rnd(st.front_back_ratio()),
                passing_side=rnd(side), passing_side_chance=rnd(chance), mean_front_gap_m=rnd(st.mean_front_gap()),
                headway_intercept_m=rnd(m), headway_slope_s=rnd(s),
                class_shares_lag0={c: rnd(p.map[0, 0, k].sum() / max(p.map[0, 0].sum(), 1))
                                   for k, c in enumerate(('standing', 'with', 'against', 'across'))})


def identifiability(sc, frames, ref_seeds, seeds):
    """stats_objective of candidates theta in THETAS against a reference ensemble made with theta = 56 on other seeds"""
    from piml_amd.calibrate import stats_objective
    from piml_amd.models.mlapm import MLAPM

    def stats(theta, sd):
        ens = MLAPM(**{**LAW, 'theta': theta}).simulate_ensemble(sc, frames, sd)
        return ens.crowd_stats(box=BOX).pooled(), ens.pair_stats().pooled(), ens.view_stats().pooled()
    ref = stats(56.0, ref_seeds)
    rows = {}
    for theta in THETAS:
        c, p, v = stats(theta, seeds)
        J2, t2 = stats_objective(c, p, ref[0], ref[1])
        J3, t3 = stats_objective(c, p, ref[0], ref[1], views=v, ref_views=ref[2])
        side, chance = v.passing_side()
        rows[f'{theta:g}'] = dict(J_crowd_pairs=round(J2, 5), J_crowd_pairs_views=round(J3, 5), J_views=round(J3 - J2, 5),
                                  front_back_ratio=round(v.front_back_ratio(), 4), passing_side=round(side, 4),
                                  passing_side_chance=round(chance, 4), mean_front_gap_m=round(v.mean_front_gap(), 4),
                                  terms={k: (None if val is None or not np.isfinite(val) else round(float(val), 5))
                                         for k, val in t3.items()})
        print(f'[viewstats] theta {theta:g}: {rows[f"{theta:g}"]}', flush=True)
    side, chance = ref[2].passing_side()
    return dict(frames=frames, reference_seeds=[ref_seeds[0], ref_seeds[-1]], candidate_seeds=[seeds[0], seeds[-1]],
                reference=dict(front_back_ratio=round(ref[2].front_back_ratio(), 4), passing_side=round(side, 4),
                               passing_side_chance=round(chance, 4), mean_front_gap_m=round(ref[2].mean_front_gap(), 4)),
                candidates=rows)


def summary(res):
    rows = ['# Heading-frame pair statistics (`piml_view_stats`, DESIGN 4.30) on one MI355X', '',
            f'`python tools/time_viewstats.py --reps {res["reps"]}` (`viewstats_time.json`): GC ensembles driven by the MLAPM '
            f'law, 750 frames, capacity {res.get("capacity")}, GC box, default options, lags 64, 128, 192; device time per '
            'call = median of 3 rounds of events around back-to-back calls, alternated with `piml_pair_stats` (defaults, the '
            'same lags and box) on the same inputs (the yardstick: the same slices and sweep).', '',
            '| input | view_stats device ms | pair_stats device ms | ratio | end to end ms | pair evaluations / s |',
            '|---|---|---|---|---|---|']
    items = [(f'GC S = {S} x 750', r) for S, r in res['gc'].items()] + [('recorded GC clip', res['recorded_gc_clip'])]
    for tag, r in items:
        rows.append(f'| {tag} | {r["device_ms"]} | {r["pair_stats_device_ms"]} | {r["ratio_to_pair_stats"]} | '
                    f'{r["end_to_end_ms"]} | {r["pair_evaluations_per_s"]:.3g} |')
    if 'findings' in res:
        rows += ['', 'What the numbers are (`findings` in `viewstats_time.json`; front/back within 2 m, passing side within '
                 '1 m, headway bins with 20 agents or more):', '',
                 '| crowd | front/back ratio | passing side | chance | mean front gap m | headway fit: gap = m + s x speed |',
                 '|---|---|---|---|---|---|']
        for k, v in res['findings'].items():
            rows.append(f'| {k} | {v["front_back_ratio"]} | {v["passing_side"]} | {v["passing_side_chance"]} | '
                        f'{v["mean_front_gap_m"]} | {v["headway_intercept_m"]} m + {v["headway_slope_s"]} s |')
    if 'identifiability' in res:
        d = res['identifiability']
        rows += ['', f'Identifiability of theta (`identifiability`): the reference is a GC ensemble under the default law '
                 f'(theta = 56), seeds {d["reference_seeds"][0]}..{d["reference_seeds"][1]}, {d["frames"]} frames; the '
                 f'candidates run seeds {d["candidate_seeds"][0]}..{d["candidate_seeds"][1]}.  `stats_objective` with the '
                 'default weights; the reference itself has front/back ratio '
                 f'{d["reference"]["front_back_ratio"]}, passing side {d["reference"]["passing_side"]} (chance '
                 f'{d["reference"]["passing_side_chance"]}).', '',
                 '| theta | J (crowd, pairs) | J (crowd, pairs, views) | view side alone | front/back ratio | passing side | '
                 'chance |', '|---|---|---|---|---|---|---|']
        for k, v in d['candidates'].items():
            rows.append(f'| {k} | {v["J_crowd_pairs"]} | {v["J_crowd_pairs_views"]} | {v["J_views"]} | '
                        f'{v["front_back_ratio"]} | {v["passing_side"]} | {v["passing_side_chance"]} |')
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--members', type=str, default='1,8,32')
    ap.add_argument('--no-findings', dest='findings', action='store_false')
    ap.add_argument('--no-identifiability', dest='identifiability', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--summary', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.viewstats import view_stats_of_raw
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(**LAW)
    res = {'frames': 750, 'reps': a.reps, 'lags': list(LAGS), 'box': list(BOX), 'gc': {}}
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        res['capacity'] = cap
        r = time_one(ens.position, ens.velocity, ens.mask_p, [min(int(n), cap) for n in ens.spawned], BOX, a.reps)
        res['gc'][str(S)] = r
        print(f'[viewstats] GC S={S} x 750 frames, cap {cap}: {r}', flush=True)
        if a.findings and S == 32:
            res.setdefault('findings', {})['mlapm_gc_ensemble_32x750'] = finding(ens.view_stats(box=BOX))
        del ens
    raws = {}
    for k, path in CLIPS.items():
        raws[k] = RawData()
        raws[k].load_trajectory_data(os.path.join(ROOT, path))
    raw = raws['gc']
    dev = lambda x: x.to('cuda').contiguous()           # noqa: E731
    r = time_one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, BOX, a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    print(f'[viewstats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents): {r}', flush=True)
    if a.findings:
        f = res.setdefault('findings', {})
        f['recorded_gc_clip_box'] = finding(view_stats_of_raw(raws['gc'], box=BOX))
        f['recorded_ucy_clip'] = finding(view_stats_of_raw(raws['ucy']))
        if 'mlapm_gc_ensemble_32x750' not in f:
            f['mlapm_gc_ensemble_32x750'] = finding(law.simulate_ensemble(sc, 750, list(range(32))).view_stats(box=BOX))
        for k, v in f.items():
            print(f'[viewstats] {k}: {v}', flush=True)
    if a.identifiability:
        res['identifiability'] = identifiability(sc, 750, list(range(100, 132)), list(range(16)))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k not in ('findings', 'identifiability')}))


if __name__ == '__main__':
    main()
