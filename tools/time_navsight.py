"""Time the any-angle floor field: its build on the GC scene beside the first-order field's, the MLAPM scenario
frame routed by the table beside the frame routed by the first-order field, and record what the obstacle and track statistics
say about GC under either.

Build: ops_scenario.nav_field(gc, cell, sight=False | True) at --cells (default 0.25, 0.125), clearance 0.3, wall time between
device synchronisations (the wall grid, the blocked cells, the goal cells on the host, the solves and their read-backs of
`changed`), the median of --reps after a warm-up, the two alternating in one process; sight=True is the first-order build plus
piml_nav_sight_relax, so the difference is the table's.  The steps queued and the grid are kept.

Frames: GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's constants with Aw = 50, Bw = -5.  `nav`
runs piml_scenario_step_mlapm_nav, whose kernels this change leaves what they were (the yardstick); `sight` the same law through
piml_scenario_step_mlapm_sight on the same seeds and the same first-order field.  Both captured (MLAPM.simulate_ensemble), by
the method of time_nav.py: per-frame cost = the difference of two runs of --frames and --short frames at one capacity, each
between device synchronisations, --reps rounds after a warm-up, the two alternating.

Findings: ObstacleStats and TrackStats of four ensembles (no wall term / Aw = 50, Bw = -5; nav / sight), recorded, not asserted.

    python tools/time_navsight.py [--reps 3] [--out profiles/navsight_time.json] [--summary profiles/navsight_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def walled(fn):
    """wall-clock milliseconds of fn between device synchronisations (the build has host work in it)"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(res):
    t = res['ms_per_frame']
    M = lambda k: f'{res["member_frames_per_s"][k] / 1e6:.2f} M'
    rounds = lambda x: ', '.join(str(v) for v in x)
    rows = ['# The any-angle floor field (`piml_nav_sight_relax`, `piml_scenario_step_mlapm_sight`, DESIGN 4.32) on one MI355X', '',
            f'`python tools/time_navsight.py --reps {res["reps"]}` (`navsight_time.json`).', '',
            '## Building the field on GC', '',
            'Wall time of `ops_scenario.nav_field(gc, cell, clearance=0.3, sight=...)` between device synchronisations; '
            f'median of {res["reps"]} after a warm-up, the two alternating.  `sight=True` is the first-order build plus '
            '`piml_nav_sight_relax` in batches of 32 launches of one Jacobi step, so the difference is the table\'s.', '',
            '| cell m | grid | gates | first-order: steps queued | ms (rounds) | with the table: sight steps queued | ms (rounds) | the table ms |',
            '|---|---|---|---|---|---|---|---|']
    for b in res['build']:
        rows.append(f'| {b["cell"]} | {b["gx"]} x {b["gy"]} | {b["G"]} | {b["steps"]} | {b["ms"]} ({rounds(b["ms_rounds"])}) | '
                    f'{b["sight_steps"]} | {b["sight_ms"]} ({rounds(b["sight_ms_rounds"])}) | {round(b["sight_ms"] - b["ms"], 3)} |')
    rows += ['', '## The frame', '',
             f'GC with `route_max_iters = 0`, {res["members"]} seeds x {res["frames"][1]} frames, capacity {res["capacity"]}, '
             f'main_mlapm.py\'s constants with Aw = 50, Bw = -5, captured; per-frame cost = the difference of a {res["frames"][1]}- '
             f'and a {res["frames"][0]}-frame run, median of {res["reps"]} rounds after a warm-up, the two alternating.  `nav` runs '
             '`scenario_mlapm_nav_kernel`, which this change left what it was.', '',
             '| frame | ms per frame (rounds) | member-frames / s | against |', '|---|---|---|---|',
             f'| nav (cell {res["nav_cell"]}) | {t["nav"]} ({rounds(res["ms_per_frame_rounds"]["nav"])}) | {M("nav")} | |',
             f'| sight | {t["sight"]} ({rounds(res["ms_per_frame_rounds"]["sight"])}) | {M("sight")} | {res["sight_over_nav"]} x nav |', '',
             'The sight lookup adds one load and two integer divisions per agent and drops nothing, so the nav frame\'s time within '
             'run-to-run spread was the expectation; the rows above are the measurement.  Kernel times were not traced.', '',
             '## What it buys (recorded, not asserted)', '',
             'All rows are GC with `route_max_iters = 0` on the same seeds.', '',
             '| GC ensemble | hit_track_fraction | contact_rate | retired | mean_straightness (complete) | persistence time s |',
             '|---|---|---|---|---|---|']
    for k, v in res['findings'].items():
        rows.append(f'| {k} | {v["hit_track_fraction"]} | {v["contact_rate"]} | {v["retired"]} of {v["spawned"]} | '
                    f'{v["mean_straightness"]} ({v["mean_straightness_complete"]}) | {v["persistence_time"]} |')
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cells', type=str, default='0.25,0.125')
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
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'members': S, 'capacity': cap, 'build': [],
           'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'member_frames_per_s': {}}
    fields = {}
    for cell in (float(x) for x in a.cells.split(',')):
        build = lambda sight: ops_scenario.nav_field(gc, cell=cell, clearance=0.3, device='cuda:0', sight=sight)
        build(False), build(True)                            # warm-up
        rounds = {False: [], True: []}
        for _ in range(a.reps):
            for sight in (False, True):
                ms, f = walled(lambda: build(sight))
                rounds[sight].append(round(ms, 3))
                fields[cell, sight] = f
        f = fields[cell, True]
        res['build'].append(dict(cell=cell, gx=f.gx, gy=f.gy, G=f.G, blocked=int(f.blocked.sum().item()), steps=f.iterations,
                                 ms=med(rounds[False]), ms_rounds=rounds[False], sight_steps=f.sight_iterations,
                                 sight_ms=med(rounds[True]), sight_ms_rounds=rounds[True]))
        print(f'[navsight] field on GC, cell {cell}: {res["build"][-1]}', flush=True)
    cell0 = max(c for c, _ in fields)                        # the coarsest (the default cell) routes the timed frames
    res['nav_cell'] = cell0
    sim = MLAPM(version='GC', **DEFAULT_INIT, Aw=50.0, Bw=-5.0)
    navs = {'nav': fields[cell0, False], 'sight': fields[cell0, True]}
    run = lambda k, T: timed(lambda: sim.simulate_ensemble(gc, T, seeds, capacity=cap, nav=navs[k]))
    per = {k: [] for k in navs}
    for k in navs:                                           # warm-up of both at the timed shapes
        run(k, a.short)
    for _ in range(a.reps):                                  # the two alternate
        for k in navs:
            per[k].append((run(k, a.frames) - run(k, a.short)) / (a.frames - a.short))
    for k in navs:
        ms = med(per[k])
        res['ms_per_frame'][k] = round(ms, 5)
        res['ms_per_frame_rounds'][k] = [round(x, 5) for x in per[k]]
        res['member_frames_per_s'][k] = round(S / ms * 1e3, 1)
    res['sight_over_nav'] = round(res['ms_per_frame']['sight'] / res['ms_per_frame']['nav'], 4)
    print(f'[navsight] GC scene, S={S}: ms per frame {res["ms_per_frame"]}, member-frames/s {res["member_frames_per_s"]}', flush=True)

    res['findings'] = {}
    plain = MLAPM(version='GC', **DEFAULT_INIT)
    r4 = lambda x: None if x is None or x != x else round(float(x), 4)
    for tag, law, k in (('no wall term, nav', plain, 'nav'), ('no wall term, sight', plain, 'sight'),
                        ('Aw = 50, Bw = -5, nav', sim, 'nav'), ('Aw = 50, Bw = -5, sight', sim, 'sight')):
        ens = law.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=navs[k])
        st, tr = ens.obstacle_stats(), ens.track_stats()
        n = [min(x, cap) for x in ens.spawned]
        retired = sum(n) - int(ens.mask_p[:, -1].sum().item())
        res['findings'][tag] = dict(hit_track_fraction=r4(st.hit_track_fraction()), contact_rate=round(st.contact_rate(), 5),
                                    mean_clearance=round(st.mean_clearance(), 3), spawned=sum(n), retired=retired,
                                    mean_straightness=r4(tr.mean_straightness()),
                                    mean_straightness_complete=r4(tr.mean_straightness('complete')),
                                    persistence_time=r4(tr.persistence_time()))
        print(f'[navsight] {tag}: {res["findings"][tag]}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
