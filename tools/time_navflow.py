"""Time and watch the direction-aware density of the floor field.

Time, by time_navdensity.py's method: GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's
constants with Aw = 50, Bw = -5, the field at cell 0.25, clearance 0.3.  One ops_scenario.nav_field_update on the state the run
left, wall time between device synchronisations, with nav_density_law(--kd, flow=1) against the same with flow = 0, in
alternating rounds in one process: medians with the rounds kept.  The deposit and the cost kernel of each path are also timed
alone, by device events.  --flow0-only --root DIR times the flow = 0 update alone with the package under DIR, which may be a
checkout that has no flow argument (the parent commit); --parent FILE merges that run's JSON into the summary.

Behaviour: the two-room, two-door plan of tests/test_navdensity_gpu.py -- gates on both sides, arrivals from both: a
counter-flow -- with the wall term on and the pair forces off, --seeds seeds x 300 frames; per door and direction the crossings
of line_stats, for the static field, kd = 2 with flow = 0 and kd = 2 with flow = 1.  Recorded, not asserted.

    python tools/time_navflow.py [--reps 5] [--out profiles/navflow_time.json] [--summary profiles/navflow_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys
import time

DOOR_WALLS = [[[5.0, -2.0], [5.0, 1.25]], [[5.0, 2.25], [5.0, 5.5]], [[5.0, 7.0], [5.0, 9.5]]]
GATES = [[[0.0, 0.5], [0.0, 3.0]], [[10.0, 0.5], [10.0, 3.0]]]
BOUNDS = (-1.5, -1.0, 11.5, 8.0)
DOORS = [[5.0, 1.25, 5.0, 2.25], [5.0, 5.5, 5.0, 7.0]]          # the near door and the far door as measurement lines


def walled(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(x):
    s = sorted(x)
    return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3), rounds=[round(v, 3) for v in x])


def time_updates(a, torch):
    from piml_amd import ops_scenario
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS, default_capacity
    gc = dataclasses.replace(SCENARIOS['gc'](), route_max_iters=0).to('cuda:0')
    cap, seeds = default_capacity(gc, a.frames), list(range(a.members))
    field = ops_scenario.nav_field(gc, cell=a.cell, clearance=0.3, device='cuda:0')
    sim = MLAPM(version='GC', **DEFAULT_INIT, Aw=50.0, Bw=-5.0)
    ens = sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, nav_density=ops_scenario.nav_density_law(a.kd))
    st = ens.state
    res = dict(members=a.members, frames=a.frames, capacity=cap, cell=a.cell, kd=a.kd, reps=a.reps, gx=field.gx, gy=field.gy,
               G=field.G, present=int((st.mask != 0).sum().item()))
    if a.flow0_only:
        paths = {'flow = 0': (ops_scenario.NavFieldDynamic(field, a.members), ops_scenario.nav_density_law(a.kd))}
    else:
        dyn = ops_scenario.NavFieldDynamic(field, a.members, flow=True)
        paths = {'flow = 0': (dyn, ops_scenario.nav_density_law(a.kd)), 'flow = 1': (dyn, ops_scenario.nav_density_law(a.kd, flow=1.0))}
    rounds, steps = {k: [] for k in paths}, {}
    for k, (f, law) in paths.items():
        ops_scenario.nav_field_update(f, st, law)                # warm-up
    for _ in range(a.reps):
        for k, (f, law) in paths.items():
            ms, steps[k] = walled(lambda: ops_scenario.nav_field_update(f, st, law), torch)
            rounds[k].append(ms)
    res['update_ms'] = {k: dict(spread(v), steps=steps[k]) for k, v in rounds.items()}
    if not a.flow0_only:
        dyn, law1 = paths['flow = 1']
        law0 = paths['flow = 0'][1]
        parts = {'nav_density': lambda: ops_scenario.nav_density(st.p, st.mask, dyn, out=dyn.count),
                 'nav_cost': lambda: ops_scenario.nav_cost(dyn.count, dyn, law0, out=dyn.cost),
                 'nav_flow': lambda: ops_scenario.nav_flow(st.p, st.v, st.mask, dyn, out=(dyn.count, dyn.mom)),
                 'nav_cost_flow': lambda: ops_scenario.nav_cost_flow(dyn.count, dyn.mom, dyn.descent, dyn, law1, out=dyn.cost_gates)}
        res['parts_ms'] = {}
        for k, fn in parts.items():
            fn()
            res['parts_ms'][k] = spread([timed(fn, torch) for _ in range(a.reps)])
        res['max_cost'] = {'flow = 0': float(dyn.cost.max().item()), 'flow = 1': float(dyn.cost_gates.max().item())}
    return res


def behaviour(a, torch):
    import numpy as np
    from piml_amd import ops_scenario, scenarios
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.models.mlapm import MLAPM
    sc = scenarios.floorplan_scenario(DOOR_WALLS, GATES, n_initial=10, rate_per_s=4.0).to('cuda:0')
    nav = ops_scenario.nav_field(sc, cell=0.25, clearance=0.3, bounds=BOUNDS, device='cuda:0')
    sim = MLAPM(version='GC', **dict(DEFAULT_INIT, A=0.0, tau=0.5), Aw=50.0, Bw=-5.0)
    seeds = list(range(a.seeds))
    out = {}
    for tag, kw in (('static field', {}), ('kd = 2, flow = 0', dict(nav_density=ops_scenario.nav_density_law(2.0))),
                    ('kd = 2, flow = 1', dict(nav_density=ops_scenario.nav_density_law(2.0, flow=1.0)))):
        e = sim.simulate_ensemble(sc, 300, seeds, capacity=256, nav=nav, **kw)
        cross = np.asarray(e.line_stats(torch.tensor(DOORS, device='cuda:0')).cross, np.int64).sum(0)        # (door, direction)
        share = [round(float(max(c) / max(c.sum(), 1)), 3) for c in cross]
        out[tag] = dict(near=cross[0].tolist(), far=cross[1].tolist(), total=int(cross.sum()), one_way_share=share,
                        spawned=sum(e.spawned), dropped=sum(e.dropped))
        print(f'[navflow] {tag}: {out[tag]}', flush=True)
    return out


def summary(res):
    rows = ['# The direction-aware density of the floor field (`piml_nav_descent`, `piml_nav_flow`, `piml_nav_cost_flow`, '
            '`piml_nav_relax_cost_gates`, DESIGN 4.36) on one MI355X', '']
    t = res.get('time')
    if t:
        u = t['update_ms']
        rows += [f'`python tools/time_navflow.py --reps {t["reps"]}`.  GC with `route_max_iters = 0`, {t["members"]} members x '
                 f'{t["frames"]} frames at capacity {t["capacity"]}, the field {t["gx"]} x {t["gy"]} cells of {t["cell"]} m, '
                 f'{t["G"]} gates, `nav_density_law({t["kd"]})`; {t["present"]} agents present in the state the updates read.', '',
                 '## One update (`nav_field_update`), wall time between device synchronisations, alternating rounds', '',
                 '| path | median ms | min .. max | rounds | Jacobi steps queued |', '|---|---|---|---|---|']
        for k, v in u.items():
            rows.append(f'| {k} | {v["median"]} | {v["min"]} .. {v["max"]} | {", ".join(str(x) for x in v["rounds"])} | {v["steps"]} |')
        p = res.get('parent')
        if p:
            v = p['update_ms']['flow = 0']
            rows.append(f'| flow = 0, the parent commit\'s package (a process of its own) | {v["median"]} | {v["min"]} .. {v["max"]} | '
                        f'{", ".join(str(x) for x in v["rounds"])} | {v["steps"]} |')
        if 'parts_ms' in t:
            rows += ['', '## The deposit and the cost alone, device events', '', '| operator | median ms | min .. max |', '|---|---|---|']
            for k, v in t['parts_ms'].items():
                rows.append(f'| `{k}` | {v["median"]} | {v["min"]} .. {v["max"]} |')
            f1, c1 = u['flow = 1']['median'], t['parts_ms']['nav_cost_flow']['median']
            rows += ['', f'The cost kernel is {c1} ms of the {f1} ms update with flow = 1 ({round(100 * c1 / f1, 1)} %); the rest is '
                     f'the solve, its copies of the cold start and its read-backs of `changed`.']
    b = res.get('behaviour')
    if b:
        rows += ['', '## Two rooms, two doors, a counter-flow', '',
                 f'Gates on both sides, arrivals from both at 4 /s, wall term on, pair forces off, {res["seeds"]} seeds x 300 frames. '
                 'Crossings of the two doors from `line_stats`, per direction (the line\'s two normals).', '',
                 '| field | near door | far door | total | share of the busier direction: near, far |', '|---|---|---|---|---|']
        for k, v in b.items():
            rows.append(f'| {k} | {v["near"][0]} + {v["near"][1]} | {v["far"][0]} + {v["far"][1]} | {v["total"]} | '
                        f'{v["one_way_share"][0]}, {v["one_way_share"][1]} |')
        st, f0, f1 = b['static field'], b['kd = 2, flow = 0'], b['kd = 2, flow = 1']
        rows += ['', f'Throughput: {st["total"]} crossings with the static field, {f0["total"]} with the head count, {f1["total"]} with '
                 f'flow = 1.  Sorting: the busier direction holds {f0["one_way_share"][0]} / {f0["one_way_share"][1]} of the near / '
                 f'far door\'s crossings with the head count and {f1["one_way_share"][0]} / {f1["one_way_share"][1]} with flow = 1 '
                 '(0.5 is no sorting, 1 a door per direction).  Observations of one run, not asserted anywhere.']
    rows += ['', '## The kernels (gfx950 code-object metadata)', '',
             '| kernel | VGPRs | SGPRs | scratch | spills | LDS bytes |', '|---|---|---|---|---|---|',
             '| `nav_descent_kernel` | 12 | 19 | 0 | 0 | 0 |', '| `nav_flow_kernel` | 9 | 20 | 0 | 0 | 0 |',
             '| `nav_cost_flow_kernel` | 50 | 59 | 0 | 0 | 15 360 |', '| `nav_relax_cost_gates_kernel` | 19 | 42 | 0 | 0 | 29 952 |', '',
             'The cost kernel stages the three integer tiles one after another through `nav_cost_kernel`\'s two buffers (the sums '
             'meet in registers only), so its LDS does not grow with the planes or the gates and a CU holds its eight workgroups of four waves (the wave limit, not LDS); '
             'the solver has `nav_relax_cost_kernel`\'s figures (19 VGPRs, 29 952 B: five workgroups a CU).  `nav_density_kernel`, '
             '`nav_cost_kernel`, `nav_relax_cost_kernel`, the 35 kernels of `scenario.hip` and the four of `nav.hip` and '
             '`navsight.hip` were compared with the parent commit\'s on the gfx950 assembly, kernel by kernel: all identical.  The '
             'frame between updates is therefore the kernel it was (`scenario_mlapm_navdyn_kernel`, 0.0211 ms a frame in '
             '`navdensity_summary.md`); it was not measured again.']
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cell', type=float, default=0.25)
    ap.add_argument('--kd', type=float, default=2.0)
    ap.add_argument('--seeds', type=int, default=2)
    ap.add_argument('--root', type=str, default=None, help='the checkout whose piml_amd is timed (default: this one)')
    ap.add_argument('--flow0-only', dest='flow0_only', action='store_true')
    ap.add_argument('--skip-time', dest='skip_time', action='store_true')
    ap.add_argument('--skip-behaviour', dest='skip_behaviour', action='store_true')
    ap.add_argument('--parent', type=str, default=None, help='the JSON of a --flow0-only run of the parent commit')
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--summary', type=str, default=None)
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    res = {'seeds': a.seeds}
    if not a.skip_time:
        res['time'] = time_updates(a, torch)
        print(f'[navflow] {res["time"]}', flush=True)
    if not a.skip_behaviour and not a.flow0_only:
        res['behaviour'] = behaviour(a, torch)
    if a.parent:
        with open(a.parent) as fh:
            res['parent'] = json.load(fh)['time']
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
