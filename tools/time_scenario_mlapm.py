"""Member-frames per second of an MLAPM-driven ensemble (MLAPM.simulate_ensemble: S seeds of one scene, one
piml_scenario_step_mlapm launch per frame, 8 frames per captured graph) for S in --members, on GC and the crosswalk at the
default capacity of --frames frames, GC law with main_mlapm.py's constants -- the method of time_scenario_ensemble.py, so
the two tables compare: per-frame cost = the difference of two runs of --frames and --short frames at one capacity
(set-up, warm-up, capture and read-back cancel), each run between device synchronisations, median of --reps alternated
pairs after a warm-up run; member-frames/s = S / per-frame cost.  Prints one JSON object.
Usage: python tools/time_scenario_mlapm.py [--scenarios gc crosswalk] [--members 1 8 32 128] [--version GC] [--reps 3]
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_scenario_mlapm.py --reps 1"""
import argparse
import json
import os
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenarios', type=str, nargs='+', default=['gc', 'crosswalk'])
    ap.add_argument('--members', type=int, nargs='+', default=[1, 8, 32, 128])
    ap.add_argument('--version', type=str, default='GC', choices=['raw', 'GC', 'UCY'])
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS, default_capacity
    law = MLAPM(version=a.version, **DEFAULT_INIT)
    med = lambda x: sorted(x)[len(x) // 2]
    res = {'law': a.version, 'frames': [a.short, a.frames], 'reps': a.reps, 'capacity': {}, 'ms_per_frame': {},
           'member_frames_per_s': {}, 'speedup_over_s1': {}}
    for name in a.scenarios:
        sc = SCENARIOS[name]().to('cuda:0')
        cap = default_capacity(sc, a.frames)
        res['capacity'][name] = cap
        for k in ('ms_per_frame', 'member_frames_per_s', 'speedup_over_s1'):
            res[k][name] = {}
        for S in a.members:
            seeds = list(range(S))
            run = lambda T: timed(lambda: law.simulate_ensemble(sc, T, seeds, capacity=cap))
            run(a.short)                                     # warm-up
            per = []
            for _ in range(a.reps):
                per.append((run(a.frames) - run(a.short)) / (a.frames - a.short))
            ms = med(per)
            res['ms_per_frame'][name][S] = round(ms, 4)
            res['member_frames_per_s'][name][S] = round(S / ms * 1e3, 1)
        base = res['member_frames_per_s'][name].get(1)
        if base:
            res['speedup_over_s1'][name] = {S: round(v / base, 2) for S, v in res['member_frames_per_s'][name].items()}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
