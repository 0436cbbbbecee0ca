"""Time the floor field: its build on the GC scene, and the MLAPM scenario frame routed by it beside the frame
with the wall term, and record what the obstacle statistics say about GC with and without the field.

Build: ops_scenario.nav_field(gc, cell) at --cells (default 0.25, 0.125), clearance 0.3, wall time between device
synchronisations (the wall grid, the blocked cells, the goal cells on the host, the solve and its read-backs of `changed`),
the median of --reps after a warm-up; the number of Jacobi steps queued and the grid are kept.

Frames: GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's constants with Aw = 50, Bw = -5.
`walls` runs the kernels of piml_scenario_step_mlapm_walls, which this change leaves what they were on the parent commit (the
yardstick); `nav` the same law through piml_scenario_step_mlapm_nav on the same seeds.  Both captured
(MLAPM.simulate_ensemble), by the method of time_noise.py: per-frame cost = the difference of two runs of --frames and --short
frames at one capacity, each between device synchronisations, --reps rounds after a warm-up, the two alternating.

Findings: ObstacleStats of the two ensembles (hit_track_fraction, contact_rate and their neighbours), recorded, not asserted.

    python tools/time_nav.py [--reps 3] [--out profiles/nav_time.json] [--summary profiles/nav_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys
import time

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

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
    rows = ['# The floor field (`piml_nav_relax`, `piml_scenario_step_mlapm_nav`, DESIGN 4.31) on one MI355X', '',
            f'`python tools/time_nav.py --reps {res["reps"]}` (`nav_time.json`).', '',
            '## Building the field on GC', '',
            'Wall time of `ops_scenario.nav_field(gc, cell, clearance=0.3)` between device synchronisations: the wall grid, the '
            'blocked cells (`wall_force` on the cell centres), the goal cells on the host, the solve in batches of 16 launches of 8 '
            f'Jacobi steps and its read-backs; median of {res["reps"]} after a warm-up.', '',
            '| cell m | grid | gates | blocked cells | steps queued | ms (rounds) |', '|---|---|---|---|---|---|']
    for b in res['build']:
        rows.append(f'| {b["cell"]} | {b["gx"]} x {b["gy"]} | {b["G"]} | {b["blocked"]} | {b["steps"]} | {b["ms"]} '
                    f'({", ".join(str(x) for x in b["ms_rounds"])}) |')
    rows += ['', '## The frame', '',
             f'GC with `route_max_iters = 0`, {res["members"]} seeds x {res["frames"][1]} frames, capacity {res["capacity"]}, '
             f'main_mlapm.py\'s constants with Aw = 50, Bw = -5, captured; per-frame cost = the difference of a {res["frames"][1]}- '
             f'and a {res["frames"][0]}-frame run, median of {res["reps"]} rounds after a warm-up, the two alternating.  `walls` '
             'runs `scenario_mlapm_walls_kernel`, whose instructions this change left what they were on the parent commit.', '',
             '| frame | ms per frame (rounds) | member-frames / s | against |', '|---|---|---|---|',
             f'| walls | {t["walls"]} ({", ".join(str(x) for x in res["ms_per_frame_rounds"]["walls"])}) | {M("walls")} | |',
             f'| walls + field (cell {res["nav_cell"]}) | {t["nav"]} ({", ".join(str(x) for x in res["ms_per_frame_rounds"]["nav"])}) | '
             f'{M("nav")} | {res["nav_over_walls"]} x walls |', '',
             'The lookup is 13 loads per agent next to a pair sum of thousands, so the routed frame was expected within a few percent '
             'of the walls frame; that was a supposition, and the row above is the measurement.  Kernel times were not traced.', '',
             '## What the obstacle statistics say (recorded, not asserted)', '',
             'All four rows are GC with `route_max_iters = 0`, so the straight-line rows also lack the pillar detour of the '
             'reference\'s scene: they are what the field replaces, not the shipped GC run.', '',
             '| GC ensemble | hit_track_fraction | contact_rate | contact_track_fraction | hit_rate | mean clearance m | retired |',
             '|---|---|---|---|---|---|---|']
    for k, v in res['findings'].items():
        rows.append(f'| {k} | {v["hit_track_fraction"]} | {v["contact_rate"]} | {v["contact_track_fraction"]} | {v["hit_rate"]} | '
                    f'{v["mean_clearance"]} | {v["retired"]} of {v["spawned"]} |')
    rows += ['', '## The pre-existing kernels', '',
             'The 20 kernels `scenario.hip` had on the parent commit (both `scenario_frame_kernel`, `scenario_route_kernel`, '
             '`scenario_groups_init_kernel`, the two plain, two walls, four groups and eight noise forms of the MLAPM frame) were '
             'compared with this tree\'s kernel by kernel on the gfx950 assembly (`hipcc --cuda-device-only -S` with `build.py`\'s '
             'flags, block labels and `.Lfunc_end` numbers normalised, each kernel\'s instructions, its `.amdhsa_kernel` block and '
             'its resource `.set` lines): 20 of 20 identical.  The other source files did not change.  New: the four '
             '`scenario_mlapm_nav_kernel<kTable, kWalls>` (74 VGPRs, no scratch, no VGPR spills, 34 816 B LDS, as the noise forms), '
             '`nav_relax_kernel` (12 VGPRs, 20 736 B LDS) and `nav_direction_kernel` (44 VGPRs).']
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
        build = lambda: ops_scenario.nav_field(gc, cell=cell, clearance=0.3, device='cuda:0')
        build()                                              # warm-up
        rounds = []
        for _ in range(a.reps):
            ms, f = walled(build)
            rounds.append(round(ms, 3))
        fields[cell] = f
        res['build'].append(dict(cell=cell, gx=f.gx, gy=f.gy, G=f.G, blocked=int(f.blocked.sum().item()), steps=f.iterations,
                                 ms=med(rounds), ms_rounds=rounds))
        print(f'[nav] field on GC, cell {cell}: {res["build"][-1]}', flush=True)
    cell0 = sorted(fields)[-1]                               # the coarsest (the default cell) routes the timed frames
    res['nav_cell'] = cell0
    sim = MLAPM(version='GC', **DEFAULT_INIT, Aw=50.0, Bw=-5.0)
    navs = {'walls': None, 'nav': fields[cell0]}
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
    res['nav_over_walls'] = round(res['ms_per_frame']['nav'] / res['ms_per_frame']['walls'], 4)
    print(f'[nav] GC scene, S={S}: ms per frame {res["ms_per_frame"]}, member-frames/s {res["member_frames_per_s"]}', flush=True)

    res['findings'] = {}
    plain = MLAPM(version='GC', **DEFAULT_INIT)
    for tag, law, nav in (('no wall term, straight lines', plain, None), ('no wall term, field', plain, fields[cell0]),
                          ('Aw = 50, Bw = -5, straight lines', sim, None), ('Aw = 50, Bw = -5, field', sim, fields[cell0])):
        ens = law.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=nav)
        st = ens.obstacle_stats()
        n = [min(x, cap) for x in ens.spawned]
        retired = sum(n) - int(ens.mask_p[:, -1].sum().item())
        res['findings'][tag] = dict(hit_track_fraction=round(st.hit_track_fraction(), 4), contact_rate=round(st.contact_rate(), 5),
                                    contact_track_fraction=round(st.contact_track_fraction(), 4), hit_rate=round(st.hit_rate(), 5),
                                    mean_clearance=round(st.mean_clearance(), 3), spawned=sum(n), retired=retired)
        print(f'[nav] {tag}: {res["findings"][tag]}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
