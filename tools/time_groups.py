"""Time the grouped clip scene of the MLAPM scenario frame beside the plain clip law, and record what group
arrivals and the group term do to the group statistics.

Scene: the recorded GC clip (tests/golden) as `clip_scenario(raw)` (law 'clip', every arrival on its own: the kernels of
piml_scenario_step_mlapm, which this change leaves instruction for instruction what they were) and as `clip_scenario(raw,
groups='auto')` (law 'clip_groups', piml_scenario_step_mlapm_groups) without the term and with Ag = 3, group_dist = 0.5.
Frames: member-frames per second of a --members-seed ensemble of each (MLAPM.simulate_ensemble, main_mlapm.py's constants,
all three at the grouped scene's default capacity of --frames frames) by the method of time_wallforce.py: per-frame cost =
the difference of two runs of --frames and --short frames at one capacity (set-up, capture and read-back cancel), each run
between device synchronisations, --reps rounds after a warm-up, the three alternating so that a busy neighbour hits all;
the median and every round are kept.
Findings: the group fraction, eligible tracks and mean member distance of the recorded clip and of the three ensembles, and
how many planted units the statistics find again.

    python tools/time_groups.py [--reps 3] [--out profiles/groups_time.json]"""
import argparse
import json
import os
import sys
import warnings

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
AG, GDIST = 3.0, 0.5                          # Moussaid et al. 2010's order of magnitude; nobody has fitted it


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def finding(st):
    rnd = lambda x: None if not np.isfinite(x) else round(float(x), 5)
    return dict(eligible_tracks=st.eligible_tracks(), links=int(st.pooled().links[0]), group_fraction=rnd(st.group_fraction()),
                mean_member_distance=rnd(st.mean_member_distance()), speed_ratio=rnd(st.speed_ratio()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import _lib
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.data.data import RawData
    from piml_amd.groupstats import group_stats_of_raw
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import clip_scenario, default_capacity
    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    rec = group_stats_of_raw(raw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        grouped = clip_scenario(raw, groups=rec.groups(0)).to('cuda:0')
    plain = clip_scenario(raw).to('cuda:0')
    cap = default_capacity(grouped, a.frames)
    sizes = grouped.row_unit[grouped.unit_rows.long(), 1].tolist()
    runs = {'clip': (MLAPM(version='GC', **DEFAULT_INIT), plain),
            'clip_groups': (MLAPM(version='GC', **DEFAULT_INIT), grouped),
            'clip_groups_term': (MLAPM(version='GC', **DEFAULT_INIT, Ag=AG, group_dist=GDIST), grouped)}
    usage = _lib.kernel_resource_usage()
    S = a.members
    seeds = list(range(S))
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'members': S, 'capacity': cap, 'group': {'Ag': AG, 'group_dist': GDIST},
           'scene': {'rows': int(grouped.entries.shape[0]), 'n_initial': grouped.n_initial, 'plain_n_initial': plain.n_initial,
                     'arrival_units': len(sizes), 'arrival_units_of_2_or_more': sum(s >= 2 for s in sizes),
                     'units_per_frame': grouped.spawn_rate, 'plain_arrivals_per_frame': plain.spawn_rate},
           'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                       for k, v in usage.items() if k.startswith(('group_force', 'scenario_groups', 'scenario_mlapm'))},
           'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'member_frames_per_s': {}}
    med = lambda x: sorted(x)[len(x) // 2]
    run = lambda k, T: timed(lambda: runs[k][0].simulate_ensemble(runs[k][1], T, seeds, capacity=cap))
    per = {k: [] for k in runs}
    for k in runs:                                           # warm-up of all three at the timed shapes
        run(k, a.short)
    for _ in range(a.reps):                                  # the three alternate
        for k in runs:
            per[k].append((run(k, a.frames) - run(k, a.short)) / (a.frames - a.short))
    for k in runs:
        ms = med(per[k])
        res['ms_per_frame'][k] = round(ms, 5)
        res['ms_per_frame_rounds'][k] = [round(x, 5) for x in per[k]]
        res['member_frames_per_s'][k] = round(S / ms * 1e3, 1)
    res['groups_over_clip'] = round(res['ms_per_frame']['clip_groups'] / res['ms_per_frame']['clip'], 4)
    res['term_over_groups'] = round(res['ms_per_frame']['clip_groups_term'] / res['ms_per_frame']['clip_groups'], 4)
    print(f'[groups] GC clip, S={S}: ms per frame {res["ms_per_frame"]}, member-frames/s {res["member_frames_per_s"]}', flush=True)
    f = {'recorded_gc_clip': finding(rec)}
    for k, (law, sc) in runs.items():
        ens = law.simulate_ensemble(sc, a.frames, seeds, capacity=cap)
        st = ens.group_stats()
        f[k] = dict(finding(st), spawned=sum(ens.spawned), dropped=sum(ens.dropped))
        if k != 'clip':
            need = st.options['min_frames'] + 1
            planted = long = found = 0
            for m in range(S):
                groups = [set(g) for g in st.groups(m)]
                for unit in ens.planted_groups(m):
                    planted += 1
                    if int((ens.mask_p[m][:, unit] == 1).all(1).sum()) >= need:
                        long += 1
                        found += any(set(unit) <= g for g in groups)
            f[k].update(planted_units=planted, present_long_enough=long, found_again=found)
        print(f'[groups] {k}: {f[k]}', flush=True)
    res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
