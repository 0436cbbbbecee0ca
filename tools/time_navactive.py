"""Time the floor-field update solved by active tiles against the update solved by batches (4.34), in one
process, the two alternating.

Scene: time_navdensity.py's -- GC with route_max_iters = 0, --members seeds x --frames frames, main_mlapm.py's constants with
Aw = 50, Bw = -5, the field at cell 0.25, clearance 0.3, nav_density_law(--kd) with its defaults.

Update: ops_scenario.nav_field_update on the state a run of --frames frames left, wall time between device
synchronisations, under solver='batch' (the reference: deposit, cost, cold-start copy, batches of 16 dense launches, a host
read per batch) and under solver='active' (the same but ONE queue of max_launches launches of piml_nav_relax_active and no
host read), --rounds rounds after a warm-up, batch and active alternating inside a round; medians and the spread
(max - min).  The fields of the two are compared bit for bit.  work: the tiles the active solve stepped, as a share of
launches x tiles x planes; `needed`: the least even number of launches whose last one changes nothing (by bisection on the
stalled word), and the active update timed at that bound too.

Runs: the --frames run, updates included, under both solvers at every = 8 and 32 (captured, the update between replays), and
under solver='active' at every = 2, captured with its frames (the batch solver cannot run that captured) and eager.

    python tools/time_navactive.py [--rounds 9] [--out profiles/navactive_time.json] [--summary profiles/navactive_summary.md]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PARENT_UPDATE_MS = 12.3                                     # one batch update of this case on the parent commit


def walled(fn):
    """wall-clock milliseconds of fn between device synchronisations"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def stats(x):
    s = sorted(x)
    return dict(ms=round(s[len(s) // 2], 3), spread=round(s[-1] - s[0], 3), rounds=[round(v, 3) for v in x])


def summary(res):
    u, r = res['update'], res['runs']
    row = lambda k, v: f'| {k} | {v["ms"]} | {v["spread"]} | {", ".join(str(x) for x in v["rounds"])} |'
    rows = ['# The floor-field update by active tiles (`piml_nav_relax_active`, DESIGN 4.37) on one MI355X', '',
            f'`python tools/time_navactive.py --rounds {res["rounds"]}` (`navactive_time.json`).  GC with `route_max_iters = 0`, '
            f'{res["members"]} seeds x {res["frames"]} frames, capacity {res["capacity"]}, main_mlapm.py\'s constants with Aw = 50, '
            f'Bw = -5, field at cell {res["cell"]} ({u["gx"]} x {u["gy"]} cells, {u["G"]} gates: {u["planes"]} planes of '
            f'{u["tiles"]} tiles), `nav_density_law(kd={res["kd"]})` with its defaults; {u["present"]} agents present.', '',
            '## One field update', '',
            'Wall time of `ops_scenario.nav_field_update` between device synchronisations on the crowd a run left; '
            f'{res["rounds"]} rounds after a warm-up, the solvers alternating inside a round; median, spread = max - min.  The '
            f'reference is the batch form, and the {PARENT_UPDATE_MS} ms DESIGN 4.34 measured for it on the parent commit.', '',
            '| update | ms | spread | rounds |', '|---|---|---|---|',
            row(f'batch ({u["batch_steps"]} steps queued, {u["batch_steps"] // 128} host reads)', u['batch']),
            row(f'active, default max_launches = {u["default_launches"]}', u['active']),
            row(f'active, max_launches = {u["needed_launches"]} (the least that converges here)', u['active_needed']), '',
            f'active / batch = {u["active_over_batch"]} (default bound), {u["needed_over_batch"]} (least bound); the fields are '
            f'{"bitwise equal" if u["same_bits"] else "DIFFERENT"}.  The active solve stepped {u["work"]} tiles: '
            f'{u["work_share_default"]} of {u["default_launches"]} launches x {u["tiles"]} tiles x {u["planes"]} planes, '
            f'{u["work_share_needed"]} of the {u["needed_launches"]} launches that were needed; the batch solve steps '
            f'{u["batch_tiles"]} (all tiles of all planes in {u["batch_steps"] // 8} launches).', '',
            '## Whole runs', '', f'{res["frames"]} frames, updates included; {res["run_rounds"]} rounds after a warm-up, alternating.', '',
            '| run | ms | spread | rounds |', '|---|---|---|---|']
    rows += [row(k, v) for k, v in r.items()]
    rows += ['', '## Not measured', '',
             'Kernel times (nothing was traced), other scenes, cell sizes and member counts, the direction-aware cost form, and '
             'the sweep.']
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--run-rounds', type=int, default=3)
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
    field = ops_scenario.nav_field(gc, cell=a.cell, clearance=0.3, device='cuda:0')
    sim = MLAPM(version='GC', **DEFAULT_INIT, Aw=50.0, Bw=-5.0)
    law = lambda solver, every=8, **kw: ops_scenario.nav_density_law(a.kd, every=every, solver=solver, **kw)
    res = {'frames': a.frames, 'rounds': a.rounds, 'run_rounds': a.run_rounds, 'members': S, 'capacity': cap, 'cell': a.cell,
           'kd': a.kd, 'parent_update_ms': PARENT_UPDATE_MS}

    # one update on the crowd of a finished run
    ens = sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, nav_density=law('batch'))
    dyn = ops_scenario.NavFieldDynamic(field, S)
    update = lambda l: ops_scenario.nav_field_update(dyn, ens.state, l)
    batch_steps = update(law('batch'))
    want = dyn.u.clone()
    default = dyn.default_max_launches()

    def converges(n):
        dyn.stalled.zero_()
        update(law('active', max_launches=n))
        return not bool(dyn.stalled.item())
    if not converges(default):
        raise SystemExit(f'the default bound of {default} launches does not converge on this case')
    same = bool(torch.equal(dyn.u.view(torch.int32), want.view(torch.int32)))
    work = int(dyn.work.sum().item())
    lo, hi = 0, default // 2                                 # the least n with converges(2 n)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if converges(2 * mid) else (mid, hi)
    needed = 2 * hi
    assert converges(needed)
    same = same and bool(torch.equal(dyn.u.view(torch.int32), want.view(torch.int32)))
    assert int(dyn.work.sum().item()) == work                # the launches past the fixed point step nothing
    kinds = {'batch': law('batch'), 'active': law('active'), 'active_needed': law('active', max_launches=needed)}
    for l in kinds.values():
        update(l)
    ms = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k, l in kinds.items():
            ms[k].append(walled(lambda: update(l))[0])
    planes, tiles = S * field.G, int(dyn.flags.shape[2] * dyn.flags.shape[3])
    u = dict(gx=field.gx, gy=field.gy, G=field.G, planes=planes, tiles=tiles, present=int((ens.state.mask != 0).sum().item()),
             batch_steps=batch_steps, batch_tiles=batch_steps // 8 * tiles * planes, default_launches=default,
             needed_launches=needed, same_bits=same, work=work, work_share_default=round(work / (default * tiles * planes), 4),
             work_share_needed=round(work / (needed * tiles * planes), 4), **{k: stats(v) for k, v in ms.items()})
    u['active_over_batch'] = round(u['active']['ms'] / u['batch']['ms'], 4)
    u['needed_over_batch'] = round(u['active_needed']['ms'] / u['batch']['ms'], 4)
    res['update'] = u
    print(f'[navactive] update: {u}', flush=True)

    # whole runs
    whole = {'static': {}, 'batch, every 32': dict(nav_density=law('batch', 32)), 'active, every 32': dict(nav_density=law('active', 32)),
             'batch, every 8': dict(nav_density=law('batch', 8)), 'active, every 8': dict(nav_density=law('active', 8)),
             'active, every 2, captured with its frames': dict(nav_density=law('active', 2)),
             'active, every 2, eager': dict(nav_density=law('active', 2), use_graph=False),
             'batch, every 2, eager': dict(nav_density=law('batch', 2), use_graph=False)}
    full = lambda k: walled(lambda: sim.simulate_ensemble(gc, a.frames, seeds, capacity=cap, nav=field, **whole[k]))[0]
    tot = {k: [] for k in whole}
    for k in whole:
        full(k)
    for _ in range(a.run_rounds):
        for k in whole:
            tot[k].append(full(k))
    res['runs'] = {k: stats(v) for k, v in tot.items()}
    print(f'[navactive] runs: {res["runs"]}', flush=True)
    for path, text in ((a.out, json.dumps(res, indent=1)), (a.summary, summary(res))):
        if path:
            with open(path, 'w') as fh:
                fh.write(text)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
