"""Time the wall term of the MLAPM scenario frame beside the plain frame, time its stand-alone operator, and
record what the term does to the obstacle statistics of the Grand Central hall.

Frames: member-frames per second of a GC ensemble of S = 1 / 8 / 32 seeds (MLAPM.simulate_ensemble at the default capacity of
--frames frames, main_mlapm.py's constants) with the wall term (Aw = 50, Bw = -5, cutoff 2 m) and without it -- the plain
frame, piml_scenario_step_mlapm, is the comparison -- by the method of time_scenario_mlapm.py: per-frame cost = the
difference of two runs of --frames and --short frames at one capacity (set-up, capture and read-back cancel), each run
between device synchronisations, --reps pairs after a warm-up, the two laws alternating so that a busy neighbour hits both;
the median and every round are kept.
Operator: piml_wall_force over the (S, frames, capacity) positions of the 32-seed ensemble, device events around --reps
back-to-back calls, median of three rounds.
Findings: the obstacle statistics of the 32-seed x 750-frame ensemble with and without the term and of the recorded GC
clip, against the same 4094 obstacle points.

    python tools/time_wallforce.py [--reps 3] [--out profiles/wallforce_time.json]"""
import argparse
import json
import os
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
AW, BW, CUTOFF = 50.0, -5.0, 2.0              # Helbing and Molnar 1995


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
    p = st.pooled()
    sp = st.speed_by_clearance()
    return dict(focal=int(p.focal[0]), steps=int(p.steps[0]), contacts=int(p.contact[0]), hits=int(p.hit[0]),
                tracks=int(p.tracks[0]), tracks_hit=int(p.tracks_hit[0]), tracks_contact=int(p.tracks_contact[0]),
                contact_rate=rnd(st.contact_rate()), hit_rate=rnd(st.hit_rate()), hit_track_fraction=rnd(st.hit_track_fraction()),
                contact_track_fraction=rnd(st.contact_track_fraction()), mean_clearance=rnd(st.mean_clearance()),
                speed_by_clearance={f'{st.r_centres[k]:.3f}': rnd(sp[k]) for k in (2, 5, 10, 20, 40, 80) if k < len(sp) - 1})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-findings', dest='findings', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import _lib, ops_scenario
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.obstaclestats import compare_obstacle_stats, obstacle_stats_of_raw
    from piml_amd.scenarios import SCENARIOS, default_capacity
    sc = SCENARIOS['gc']().to('cuda:0')
    cap = default_capacity(sc, a.frames)
    laws = {'plain': MLAPM(version='GC', **DEFAULT_INIT),
            'walls': MLAPM(version='GC', **DEFAULT_INIT, Aw=AW, Bw=BW, wall_cutoff=CUTOFF)}
    grid = ops_scenario.wall_grid(sc.obstacles, CUTOFF, 'cuda:0')
    nb = np.diff(grid.host.cell_start).reshape(grid.gy, grid.gx)
    pad = np.pad(nb, 1)
    nb9 = sum(pad[1 + dy:1 + dy + grid.gy, 1 + dx:1 + dx + grid.gx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    usage = _lib.kernel_resource_usage()
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'capacity': cap, 'wall': {'Aw': AW, 'Bw': BW, 'cutoff': CUTOFF},
           'grid': {'points': grid.n_points, 'gx': grid.gx, 'gy': grid.gy, 'cell': grid.cell,
                    'fullest_3x3_neighbourhood': int(nb9.max())},
           'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                       for k, v in usage.items() if k.startswith(('wall_force', 'scenario_mlapm'))},
           'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'member_frames_per_s': {}, 'walls_over_plain': {}}
    med = lambda x: sorted(x)[len(x) // 2]
    for S in a.members:
        seeds = list(range(S))
        run = lambda law, T: timed(lambda: law.simulate_ensemble(sc, T, seeds, capacity=cap))
        per = {k: [] for k in laws}
        for law in laws.values():                            # warm-up of both at the timed shapes
            run(law, a.short)
        for _ in range(a.reps):                              # the two alternate
            for k, law in laws.items():
                per[k].append((run(law, a.frames) - run(law, a.short)) / (a.frames - a.short))
        for k in laws:
            ms = med(per[k])
            res['ms_per_frame'].setdefault(k, {})[S] = round(ms, 5)
            res['ms_per_frame_rounds'].setdefault(k, {})[S] = [round(x, 5) for x in per[k]]
            res['member_frames_per_s'].setdefault(k, {})[S] = round(S / ms * 1e3, 1)
        res['walls_over_plain'][S] = round(res['ms_per_frame']['walls'][S] / res['ms_per_frame']['plain'][S], 4)
        print(f'[wallforce] GC S={S}: ms per frame {({k: res["ms_per_frame"][k][S] for k in laws})}, member-frames/s '
              f'{({k: res["member_frames_per_s"][k][S] for k in laws})}', flush=True)
    S = max(a.members)
    ens = {k: law.simulate_ensemble(sc, a.frames, list(range(S)), capacity=cap) for k, law in laws.items()}
    pos = ens['walls'].position.contiguous()
    call = lambda: ops_scenario.wall_force(pos, grid, AW, BW)
    for _ in range(2):
        force = call()
    rounds = []
    for _ in range(3):
        rounds.append(timed(lambda: [call() for _ in range(a.reps)]) / a.reps)
    present = int((ens['walls'].mask_p == 1).sum())
    felt = int(((force != 0).any(-1) & (ens['walls'].mask_p == 1)).sum())
    res['operator'] = {'shape': list(pos.shape[:-1]), 'rows': pos.numel() // 2, 'present_rows': present, 'rows_with_a_force': felt,
                       'ms': round(med(rounds), 4), 'ms_rounds': [round(x, 4) for x in rounds],
                       'rows_per_s': float(f'{pos.numel() // 2 / (med(rounds) * 1e-3):.4g}')}
    print(f'[wallforce] operator over {tuple(pos.shape[:-1])}: {res["operator"]}', flush=True)
    if a.findings:
        raw = RawData()
        raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
        rec = obstacle_stats_of_raw(raw, sc.obstacles)
        f = {'recorded_gc_clip': finding(rec)}
        for k, e in ens.items():
            st = e.obstacle_stats()
            f[f'mlapm_{k}_gc_ensemble_{S}x{a.frames}'] = finding(st)
            f[f'mlapm_{k}_gc_ensemble_{S}x{a.frames}_vs_recorded'] = {
                n: (None if isinstance(v, float) and not np.isfinite(v) else v) for n, v in compare_obstacle_stats(st, rec).items()}
        for k, v in f.items():
            print(f'[wallforce] {k}: {v}', flush=True)
        res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
