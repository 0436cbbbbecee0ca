"""Time the exit choice: the routed MLAPM frame with the choice launch in front of it beside the frame alone, and
what the exits and the measurement lines say about GC with and without the choice.

Scene: GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's constants with Aw = 50, Bw = -5, the
field at cell 0.25, clearance 0.3, captured (8 frames a graph); two of GC's right-hand gates, 3 and 4, are one class, the law is
exit_choice_law([[3, 4]]) with its defaults but for `every`.

Frames: `nav` is the static routed frame (piml_scenario_step_mlapm_nav, which this change leaves what it was on the parent
commit: the yardstick); `nav + choice` the same frame with piml_nav_choose_exit in front, at every = 8 (seven launches in
eight return at once) and at every = 1; `navdyn` and `navdyn + choice` the same pair under nav_density with an update interval
longer than the run, so that both timed runs hold exactly one update, which the difference removes.  Per-frame cost = the
difference of two captured runs of --frames and --short frames at one capacity, by the method of time_navdensity.py, the
kinds alternating; the median of --reps rounds.

Findings: retired agents per gate, switches, and the mean travel time between two measurement lines, recorded, not asserted.

    python tools/time_navchoice.py [--reps 9] [--out profiles/navchoice_time.json] [--summary profiles/navchoice_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LINES = [[2.0, 5.0, 2.0, 17.0], [28.0, 5.0, 28.0, 35.0]]         # inside the left gate, inside the right-hand gates
CLASSES = [[3, 4]]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(res):
    t, r = res['ms_per_frame'], res['ms_per_frame_rounds']
    rows = ['# The exit choice (`piml_nav_choose_exit`, DESIGN 4.35) on one MI355X', '',
            f'`python tools/time_navchoice.py --reps {res["reps"]}` (`navchoice_time.json`).  GC with `route_max_iters = 0`, '
            f'{res["members"]} seeds x {res["frames"][1]} frames, capacity {res["capacity"]}, main_mlapm.py\'s constants with '
            f'Aw = 50, Bw = -5, field at cell {res["cell"]}, captured; gates {res["classes"]} one class, '
            '`exit_choice_law` with its defaults but for `every`.', '',
            '## The frame with the choice launch in front', '',
            f'Per-frame cost = the difference of a {res["frames"][1]}- and a {res["frames"][0]}-frame captured run, median of '
            f'{res["reps"]} rounds after a warm-up, the kinds alternating.  `nav` runs `scenario_mlapm_nav_kernel`, whose '
            'instructions this change left what they were on the parent commit; the `navdyn` rows hold one field update in each '
            'run, which the difference removes.', '', '| frame | ms per frame (rounds) | against |', '|---|---|---|']
    for k, base in (('nav', None), ('nav + choice, every 8', 'nav'), ('nav + choice, every 1', 'nav'), ('navdyn', None),
                    ('navdyn + choice, every 8', 'navdyn')):
        ratio = '' if base is None else f'{round(t[k] / t[base], 4)} x {base}, {round((t[k] - t[base]) * 1e3, 2)} us more'
        rows.append(f'| {k} | {t[k]} ({", ".join(str(x) for x in r[k])}) | {ratio} |')
    rows += ['', '## What the exits say (recorded, not asserted)', '',
             f'Retired agents per gate over all members, the switches made, and the mean travel time from line 0 to line 1 of '
             f'{res["lines"]} (`line_stats`, seconds).', '',
             '| GC ensemble | retired per gate 0 .. 6 | switches | travel time 0 -> 1 | 1 -> 0 | retired |', '|---|---|---|---|---|---|']
    for k, v in res['findings'].items():
        rows.append(f'| {k} | {v.get("exits")} | {v.get("switches")} | {v.get("travel_01")} | {v.get("travel_10")} | '
                    f'{v.get("retired")} of {v.get("spawned")} |' if 'error' not in v else f'| {k} | {v["error"]} | | | | |')
    rows += ['', '## The pre-existing kernels', '',
             'The kernel lives in `scenario.hip`, beside the spawn helpers it shares.  The 34 kernels that file had on the parent '
             'commit were compared with this tree\'s kernel by kernel on the gfx950 assembly (`hipcc -S --cuda-device-only` with '
             '`build.py`\'s flags, block labels and `.Lfunc_end` numbers normalised, comments dropped; each kernel\'s instructions '
             'and its `.amdhsa_kernel` block): 34 of 34 identical.  New: `scenario_choose_exit_kernel`, 38 VGPRs, 56 SGPRs, no '
             'scratch, no spills, no LDS.', '',
             '## Not measured', '',
             'Kernel times (nothing was traced), other class sizes, member counts and cell sizes, the network-driven frame, the '
             'sweep.  The parent commit\'s frame was not run from a checkout of its own: its kernels are in this library '
             'instruction for instruction, and `nav` above is that frame.']
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=9)
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
    choice = lambda every: ops_scenario.exit_choice_law(CLASSES, every=every)
    never = (a.frames // 8 + 1) * 8                          # a multiple of frames_per_graph longer than the run: one update at t = 1
    dens = ops_scenario.nav_density_law(a.kd, every=never)
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'members': S, 'capacity': cap, 'cell': a.cell, 'kd': a.kd, 'lines': LINES,
           'classes': CLASSES, 'ms_per_frame': {}, 'ms_per_frame_rounds': {}}
    kinds = {'nav': {}, 'nav + choice, every 8': dict(exit_choice=choice(8)), 'nav + choice, every 1': dict(exit_choice=choice(1)),
             'navdyn': dict(nav_density=dens), 'navdyn + choice, every 8': dict(nav_density=dens, exit_choice=choice(8))}
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
    print(f'[navchoice] ms per frame {res["ms_per_frame"]}', flush=True)

    res['findings'] = {}
    live = ops_scenario.nav_density_law(a.kd, every=8)
    for tag, kw in (('static field', {}), ('static field + choice', dict(exit_choice=choice(8))),
                    (f'kd = {a.kd}', dict(nav_density=live)), (f'kd = {a.kd} + choice', dict(nav_density=live, exit_choice=choice(8)))):
        e = sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, **kw)
        n = [min(x, cap) for x in e.spawned]
        row = dict(spawned=sum(n), retired=sum(n) - int(e.mask_p[:, -1].sum().item()),
                   exits=np.asarray(e.exit_counts()).sum(0).tolist(),
                   switches=None if e.exit_switches is None else int(e.exit_switches.sum().item()))
        try:
            tt = np.asarray(e.line_stats(torch.tensor(LINES, device='cuda:0')).mean_travel_time(), np.float64)
            row.update(travel_01=None if not np.isfinite(tt[0, 1]) else round(float(tt[0, 1]), 3),
                       travel_10=None if not np.isfinite(tt[1, 0]) else round(float(tt[1, 0]), 3))
        except Exception as ex:                              # the timings above are kept; the row says what went wrong
            row['error'] = f'{type(ex).__name__}: {ex}'
        res['findings'][tag] = row
        print(f'[navchoice] {tag}: {row}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
