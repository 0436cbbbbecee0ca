"""Time the density-aware floor field: one field update, the frame between updates beside the static routed
frame, whole runs at two update intervals, and what the measurement lines and the fundamental diagram say about GC with and
without the term.

Scene: GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's constants with Aw = 50, Bw = -5, the
field at cell 0.25, clearance 0.3; the density law is nav_density_law(--kd) with its defaults.

Update: ops_scenario.nav_field_update on the state a run of --frames frames left (the crowd of the last frame), wall time
between device synchronisations -- the deposit, the cost, the copy of the cold start, the solve in batches of 16 launches and its
read-backs of `changed` --, the median of --reps after a warm-up; the Jacobi steps queued are kept.

Frames: `nav` is the static routed frame (piml_scenario_step_mlapm_nav, which this change leaves what it was on the parent
commit: the yardstick); `navdyn` the frame with a field per member (piml_scenario_step_mlapm_navdyn) under a law whose `every`
is longer than the run, so that both timed runs hold exactly one update, which the difference removes.  Per-frame cost = the
difference of two captured runs of --frames and --short frames at one capacity, by the method of time_nav.py, the two
alternating.  Whole runs: the time of a --frames run, updates included, at every = 8 and 32, beside the static run.

Findings: flow over two measurement lines and the pooled speed and density of crowd_stats, recorded, not asserted.

    python tools/time_navdensity.py [--reps 3] [--out profiles/navdensity_time.json] [--summary profiles/navdensity_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LINES = [[0.0, 2.0, 30.0, 2.0], [2.0, 5.0, 2.0, 17.0]]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def walled(fn):
    """wall-clock milliseconds of fn between device synchronisations (the update has host reads in it)"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(res):
    t, u = res['ms_per_frame'], res['update']
    rows = ['# The density-aware floor field (`piml_nav_density`, `piml_nav_cost`, `piml_nav_relax_cost`, '
            '`piml_scenario_step_mlapm_navdyn`, DESIGN 4.34) on one MI355X', '',
            f'`python tools/time_navdensity.py --reps {res["reps"]}` (`navdensity_time.json`).  GC with `route_max_iters = 0`, '
            f'{res["members"]} seeds x {res["frames"][1]} frames, capacity {res["capacity"]}, main_mlapm.py\'s constants with '
            f'Aw = 50, Bw = -5, field at cell {res["cell"]} ({u["gx"]} x {u["gy"]} cells, {u["G"]} gates), '
            f'`nav_density_law(kd={res["kd"]})` with its defaults.', '',
            '## One field update', '',
            'Wall time of `ops_scenario.nav_field_update` between device synchronisations on the crowd a run left: deposit, cost, '
            'the copy of the cold start, the solve in batches of 16 launches of 8 steps and one host read of `changed` per batch; '
            f'median of {res["reps"]} after a warm-up.', '',
            '| members | planes | steps queued | ms (rounds) | present agents |', '|---|---|---|---|---|',
            f'| {res["members"]} | {res["members"] * u["G"]} | {u["steps"]} | {u["ms"]} ({", ".join(str(x) for x in u["ms_rounds"])}) | '
            f'{u["present"]} |', '',
            '## The frame between updates', '',
            f'Per-frame cost = the difference of a {res["frames"][1]}- and a {res["frames"][0]}-frame captured run, median of '
            f'{res["reps"]} rounds after a warm-up, the two alternating.  `nav` runs `scenario_mlapm_nav_kernel`, whose instructions '
            'this change left what they were on the parent commit; `navdyn` holds one update in each run, which the difference removes.',
            '', '| frame | ms per frame (rounds) | against |', '|---|---|---|',
            f'| nav (static field) | {t["nav"]} ({", ".join(str(x) for x in res["ms_per_frame_rounds"]["nav"])}) | |',
            f'| navdyn (field per member) | {t["navdyn"]} ({", ".join(str(x) for x in res["ms_per_frame_rounds"]["navdyn"])}) | '
            f'{res["navdyn_over_nav"]} x nav |', '',
            '## Whole runs', '', f'{res["frames"][1]} frames, updates and their host reads included; median of {res["reps"]} rounds.', '',
            '| run | ms (rounds) | member-frames / s | against |', '|---|---|---|---|']
    for k, v in res['runs'].items():
        rows.append(f'| {k} | {v["ms"]} ({", ".join(str(x) for x in v["ms_rounds"])}) | {v["member_frames_per_s"] / 1e6:.3f} M | '
                    f'{v["over_static"]} x static |')
    rows += ['', '## What the statistics say (recorded, not asserted)', '',
             f'Flow over the lines {res["lines"]} (crossings per second, both directions summed) and the pooled mean speed and '
             'density of `crowd_stats`.', '', '| GC ensemble | flow line 0 | flow line 1 | mean speed m/s | mean density 1/m^2 | retired |',
             '|---|---|---|---|---|---|']
    for k, v in res['findings'].items():
        rows.append(f'| {k} | {v.get("flow0")} | {v.get("flow1")} | {v.get("mean_speed")} | {v.get("mean_density")} | '
                    f'{v.get("retired")} of {v.get("spawned")} |' if 'error' not in v else f'| {k} | {v["error"]} | | | | |')
    rows += ['', 'GC has no bottleneck to speak of: the term spreads the crowd a little and costs a little speed and throughput to '
             'detours.  The update is the whole cost of a run with the term; the frame between updates is level with the static '
             'routed frame, whose lookup it shares (the two runs differ in where the agents are).', '',
             '## Two rooms and two doors (`tests/test_navdensity_gpu.py`)', '',
             'Near door 1 m wide straight between the gates, far door a detour; pair forces off, Aw = 50, Bw = -5, cell 0.25, the '
             'default law but for kd, 2 seeds x 300 frames, crossings of the wall\'s line.  First run, from which the test\'s rate '
             'and kd were chosen (4 arrivals a second, kd = 2):', '',
             '| arrivals / s | kd | crossings | near door | far door (share) | outside both |', '|---|---|---|---|---|---|',
             '| 4 | static | 151 | 151 | 0 | 0 |', '| 4 | 0.5 | 149 | 103 | 46 (0.31) | 0 |', '| 4 | 1 | 139 | 80 | 59 (0.42) | 0 |',
             '| 4 | 2 | 126 | 62 | 64 (0.51) | 0 |', '| 4 | 4 | 109 | 53 | 56 (0.51) | 0 |', '| 8 | static | 307 | 307 | 0 | 0 |',
             '| 8 | 0.5 | 283 | 164 | 119 (0.42) | 0 |', '| 8 | 1 | 268 | 136 | 132 (0.49) | 0 |', '| 8 | 2 | 240 | 116 | 124 (0.52) | 0 |',
             '| 8 | 4 | 228 | 116 | 112 (0.49) | 0 |', '',
             'Fewer agents cross in 300 frames as kd grows: they re-decide at every update and dither.  Without the wall term an '
             'agent whose field turns under it can be carried into the blocked band beside the wall, where the lookup is the '
             'straight line: at 4 arrivals a second 15 / 18 / 26 / 25 of 165 / 157 / 139 / 123 crossings lay outside both doors for '
             'kd = 1 / 2 / 4 / 8 (none with the static field).', '',
             '## The pre-existing kernels', '',
             'The 30 kernels `scenario.hip` had on the parent commit were compared with this tree\'s kernel by kernel on the gfx950 '
             'assembly (`hipcc --save-temps` with `build.py`\'s flags, block labels and `.Lfunc_end` numbers normalised, each kernel\'s '
             'instructions and its `.amdhsa_kernel` block): 30 of 30 identical, and `-Rpass-analysis=kernel-resource-usage` gives '
             'every one of them the registers, spills, scratch, occupancy and LDS it had.  `nav.hip` did not change.  New: the four '
             '`scenario_mlapm_navdyn_kernel<kTable, kWalls>` (74 VGPRs, 106 SGPRs, no scratch, no VGPR spills, 34 816 B LDS, 4 waves a '
             'SIMD, as the nav forms), `nav_relax_cost_kernel` (19 VGPRs, 29 952 B LDS: 5 workgroups a CU against `nav_relax_kernel`\'s '
             '7), `nav_cost_kernel` (50 VGPRs, 15 360 B LDS) and `nav_density_kernel` (7 VGPRs).', '',
             '## Not measured', '',
             'Kernel times (nothing was traced), other cell sizes and member counts, the sweep, the update with fewer launches per '
             'batch.  The parent commit\'s frame was not run from a checkout of its own: its kernels are in this library instruction '
             'for instruction, and `nav` above is that frame.']
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cell', type=float, default=0.25)
    ap.add_argument('--kd', type=float, default=2.0)
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--summary', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import ops_scenario
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS, default_capacity
    gc = dataclasses.replace(SCENARIOS['gc'](), route_max_iters=0).to('cuda:0')
    cap = default_capacity(gc, a.frames)
    S = a.members
    seeds = list(range(S))
    med = lambda x: sorted(x)[len(x) // 2]
    field = ops_scenario.nav_field(gc, cell=a.cell, clearance=0.3, device='cuda:0')
    sim = MLAPM(version='GC', **DEFAULT_INIT, Aw=50.0, Bw=-5.0)
    law = lambda every: ops_scenario.nav_density_law(a.kd, every=every)
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'members': S, 'capacity': cap, 'cell': a.cell, 'kd': a.kd, 'lines': LINES,
           'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'runs': {}}

    # one update on the crowd of a finished run
    ens = sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, nav_density=law(8))
    dyn = ops_scenario.NavFieldDynamic(field, S)
    update = lambda: ops_scenario.nav_field_update(dyn, ens.state, law(8))
    update()
    rounds = []
    for _ in range(a.reps):
        ms, steps = walled(update)
        rounds.append(round(ms, 3))
    res['update'] = dict(gx=field.gx, gy=field.gy, G=field.G, steps=steps, ms=med(rounds), ms_rounds=rounds,
                         present=int((ens.state.mask != 0).sum().item()), max_cost=float(dyn.cost.max().item()))
    print(f'[navdensity] update: {res["update"]}', flush=True)

    # the frame between updates
    never = (a.frames // 8 + 1) * 8                          # a multiple of frames_per_graph longer than the run: one update at t = 1
    kinds = {'nav': {}, 'navdyn': dict(nav_density=law(never))}
    run = lambda k, T: timed(lambda: sim.simulate_ensemble(gc, T, seeds, capacity=cap, nav=field, **kinds[k]))
    per = {k: [] for k in kinds}
    for k in kinds:
        run(k, a.short)
    for _ in range(a.reps):
        for k in kinds:
            per[k].append((run(k, a.frames) - run(k, a.short)) / (a.frames - a.short))
    for k in kinds:
        res['ms_per_frame'][k] = round(med(per[k]), 5)
        res['ms_per_frame_rounds'][k] = [round(x, 5) for x in per[k]]
    res['navdyn_over_nav'] = round(res['ms_per_frame']['navdyn'] / res['ms_per_frame']['nav'], 4)
    print(f'[navdensity] ms per frame {res["ms_per_frame"]}', flush=True)

    # whole runs
    whole = {'static': {}, 'every 32': dict(nav_density=law(32)), 'every 8': dict(nav_density=law(8))}
    tot = {k: [] for k in whole}
    full = lambda k: walled(lambda: sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, **whole[k]))[0]
    for k in whole:
        full(k)
    for _ in range(a.reps):
        for k in whole:
            tot[k].append(round(full(k), 3))
    for k in whole:
        ms = med(tot[k])
        res['runs'][k] = dict(ms=ms, ms_rounds=tot[k], member_frames_per_s=round(S * (a.frames - 1) / ms * 1e3, 1))
    for k in whole:
        res['runs'][k]['over_static'] = round(res['runs'][k]['ms'] / res['runs']['static']['ms'], 4)
    print(f'[navdensity] runs {res["runs"]}', flush=True)

    res['findings'] = {}
    for tag, kw in (('static field', {}), (f'kd = {a.kd}, every 8', dict(nav_density=law(8))),
                    (f'kd = {a.kd}, every 32', dict(nav_density=law(32)))):
        e = sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, **kw)
        n = [min(x, cap) for x in e.spawned]
        row = dict(spawned=sum(n), retired=sum(n) - int(e.mask_p[:, -1].sum().item()))
        try:
            ls = e.line_stats(torch.tensor(LINES, device='cuda:0'))
            flow = np.asarray(ls.flow(), np.float64).sum(-1)
            cs = e.crowd_stats()
            row.update(flow0=round(float(flow[0]), 4), flow1=round(float(flow[1]), 4),
                       mean_speed=round(float(np.nanmean(np.asarray(cs.mean_speed, np.float64))), 4),
                       mean_density=round(float(np.nanmean(np.asarray(cs.mean_density, np.float64))), 4),
                       fd_mean=[None if not np.isfinite(x) else round(float(x), 4)
                                for x in np.nanmean(np.asarray(cs.fd_mean, np.float64), 0)])
        except Exception as ex:                              # the timings above are kept; the row says what went wrong
            row['error'] = f'{type(ex).__name__}: {ex}'
        res['findings'][tag] = row
        print(f'[navdensity] {tag}: {row}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
