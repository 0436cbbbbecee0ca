"""ms per simulated frame of the open-world scenario (BaseSimulator.simulate_scenario on a scene of
piml_amd.scenarios.SCENARIOS, default gc, one captured frame replayed) at N = capacity, pinnsf_m in eval mode; for GC against
the clip rollout's frame (get_multiple_rollouts on the synthetic GC clip of piml_amd.scenes with the same obstacle points).  Per-frame cost = the difference of two runs of
different lengths (set-up, warm-up and capture cancel), median of --reps alternated pairs.
Prints one JSON object.  Usage: python tools/time_scenario.py [--scenario NAME] [--caps 256 1024 4096] [--reps 5]
--routed: the frame under the floor field instead.  GC with route_max_iters = 0 at every capacity three ways, the
three alternating inside every repetition of one run: `none` without a field -- piml_scenario_step_members, the entry the frame
had before the field and which the routed work does not touch: the baseline --, `field` (simulate_scenario(nav=nav_field(gc)),
piml_scenario_step_nav) and `sight` (the field with its any-angle table).  [--out FILE.json] keeps the JSON.
Kernel list of a frame: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_scenario.py --caps 1024 --reps 1"""
import argparse
import json
import os
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def routed(a):
    import dataclasses
    from test_simulator_gpu import sim_args
    from piml_amd import ops_scenario
    from piml_amd.models.simulators import BaseSimulator
    from piml_amd.scenarios import SCENARIOS
    torch.manual_seed(0)
    sim = BaseSimulator(sim_args())
    sim.model.eval()
    sc = dataclasses.replace(SCENARIOS['gc'](), route_max_iters=0).to('cuda:0')
    field = ops_scenario.nav_field(sc, device='cuda:0', sight=True)
    plain = ops_scenario.NavField(field.u, field.blocked, field.goal, field.x0, field.y0, field.cell, field.near, field.clearance,
                                  field.iterations)                  # the same planes without the table
    navs = {'none': None, 'field': plain, 'sight': field}
    med = lambda x: sorted(x)[len(x) // 2]
    res = {'scenario': 'gc, route_max_iters = 0', 'frames': [a.short, a.long], 'reps': a.reps,
           'grid': [field.gx, field.gy, field.G], 'cell': field.cell, 'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'ratio': {},
           'agents_present_last_frame': {}}
    for cap in a.caps:
        run = lambda k, T: timed(lambda: sim.simulate_scenario(sc, T, seed=1, capacity=cap, nav=navs[k]))
        per = {k: [] for k in navs}
        with torch.no_grad():
            for k in navs:                                   # warm-up of each at the timed capacity
                run(k, a.short)
            for _ in range(a.reps):                          # the three alternate: the host is shared
                for k in navs:
                    per[k].append((run(k, a.long) - run(k, a.short)) / (a.long - a.short))
            last = {k: sim.simulate_scenario(sc, a.long, seed=1, capacity=cap, nav=navs[k]) for k in navs}
        res['ms_per_frame'][cap] = {k: round(med(per[k]), 4) for k in navs}
        res['ms_per_frame_rounds'][cap] = {k: [round(x, 4) for x in per[k]] for k in navs}
        res['ratio'][cap] = {k: round(med(per[k]) / med(per['none']), 3) for k in ('field', 'sight')}
        res['agents_present_last_frame'][cap] = {k: int(last[k].mask_p[-1].sum().item()) for k in navs}
        print(f'[routed] capacity {cap}: {res["ms_per_frame"][cap]} ms per frame, against none {res["ratio"][cap]}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenario', type=str, default='gc')
    ap.add_argument('--caps', type=int, nargs='+', default=[256, 1024, 4096])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--short', type=int, default=40)
    ap.add_argument('--long', type=int, default=240)
    ap.add_argument('--routed', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    if a.routed:
        return routed(a)
    from test_simulator_gpu import sim_args
    from piml_amd.models.simulators import BaseSimulator
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.scenes import synthetic_rollout_data
    torch.manual_seed(0)
    sim = BaseSimulator(sim_args())
    sim.model.eval()
    sc = SCENARIOS[a.scenario]().to('cuda:0')
    gc = a.scenario == 'gc'
    M = sc.obstacles.shape[0]
    res = {'scenario': a.scenario, 'frames': [a.short, a.long], 'reps': a.reps, 'obstacles': M, 'scenario_ms_per_frame': {}, 'rollout_ms_per_frame': {},
           'ratio': {}, 'agents_present_last_frame': {}}
    for cap in a.caps:
        clips = {T: synthetic_rollout_data(cap, M, T, 'cuda:0', seed=1) for T in (a.short, a.long)} if gc else None

        def scen(T):
            return timed(lambda: sim.simulate_scenario(sc, T, seed=1, capacity=cap))

        def roll(T):
            return timed(lambda: sim.get_multiple_rollouts(clips[T], t_start=0, load_model=False))

        with torch.no_grad():
            scen(a.short), gc and roll(a.short)              # warm-up
            s, r = [], []
            for _ in range(a.reps):                          # alternated: the host is shared
                s.append((scen(a.long) - scen(a.short)) / (a.long - a.short))
                if gc:
                    r.append((roll(a.long) - roll(a.short)) / (a.long - a.short))
            last = sim.simulate_scenario(sc, a.long, seed=1, capacity=cap)
        med = lambda x: sorted(x)[len(x) // 2]
        res['scenario_ms_per_frame'][cap] = round(med(s), 4)
        if gc:
            res['rollout_ms_per_frame'][cap] = round(med(r), 4)
            res['ratio'][cap] = round(med(s) / med(r), 3)
        res['agents_present_last_frame'][cap] = int(last.mask_p[-1].sum().item())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
