"""GPU: whole routed MLAPM runs, frame by frame and update by update (scenario_mlapm_body with kNav, kSight and the per-member
navdyn form inside MLAPM._run_scenario's schedule).  The test drives the run itself with the public primitives, in the order
_run_scenario's docstring states (tests/mlapm_routed_twin.py): every frame is compared with a twin stepped WITHOUT the field on a
state whose destination was overwritten by p + e of ops_scenario.nav_direction; every field update with the numpy restatements
on the positions the run handed it; every exit choice with navchoice_ref on the state and field of that moment; and the loop's
result with MLAPM.simulate_ensemble eager and captured (simulate_sweep for the table form), which carries the per-frame checks
over to the product loop.  Every comparison is bitwise but e against the host lookup (1e-5, the lookup tests' tolerance).

Sizes.  The static forms run the 200 frames the network-driven twin runs.  The forms with a dynamic field run 160 frames:
on the plan the way from gate to gate is about 11 m through the door, 100 frames at 1.34 m/s, so a run of 60 frames retires
nobody and the assertions that every member retires an agent and shows a slot retired for good could not hold; 160 frames
give updates at 1, 9, .., 153 (every 8) and 1, 5, .., 157 (every 4).  The exit-choice form runs the hall of
test_navchoice_gpu.py -- the floor plan with one class of two equivalent exits that file's runs switch on -- with the kd = 2 and
the choice law its runs and profiles/navchoice_summary.md record as switching.  On that hall as its arrivals fill it the field
of before an update never chooses otherwise than the fresh one, so a further case plants a queue at the near exit and probes
where the exits are equally far (_plant_the_queue): there the two fields choose differently for every probe, and the order of
update and choice shows in the test's loop and in the product's."""
import functools

import numpy as np
import pytest
import torch

import mlapm_routed_twin as TWIN
import nav_ref
from test_scenario_mlapm_gpu import _same, bits
from test_scenario_nav_gpu import BOUNDS, NOISY, PLAIN, SEEDS, WALLED, field, scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T_STATIC, T_DYNAMIC = 200, 160
# the counter values t = 0 .. T-2 with t >= 1 and (t - 1) % every == 0, written out (T = 60, every = 8: 1, 9, .., 57)
EVERY_8 =[1, 9, 17, 25, 33, 41, 49, 57, 65, 73, 81, 89, 97, 105, 113, 121, 129, 137, 145, 153]
EVERY_4 = [1, 5, 9, 13, 17, 21, 25, 29, 33, 37, 41, 45, 49, 53, 57, 61, 65, 69, 73, 77, 81, 85, 89, 93, 97, 101, 105, 109, 113,
           117, 121, 125, 129, 133, 137, 141, 145, 149, 153, 157]
LEFT_OUT_CAP = 0.05                                              # of the routed live rows: those the frame retired in A


@functools.lru_cache(maxsize=None)
def sight_field():
    from piml_amd import ops_scenario
    return ops_scenario.nav_field(scene('plan'), cell=0.25, clearance=0.3, bounds=BOUNDS, device=DEV, sight=True)


def _density(kd=4.0, rho0=0.0, **kw):
    from piml_amd import ops_scenario
    return ops_scenario.nav_density_law(kd, rho0=rho0, **kw)


def _plan():
    return scene('plan'), field('plan')


def _sight():
    return scene('plan'), sight_field()


def _hall():
    from test_navchoice_gpu import hall, hall_field
    return hall(), hall_field()


def _choice():
    from piml_amd import ops_scenario
    return ops_scenario.exit_choice_law([[1, 2]], margin=1.0, commit=1.0, every=8)


# name: where, law, T, capacity, and what the form adds
FORMS = {
    'static': dict(where=_plan, params=PLAIN, T=T_STATIC, cap=64),
    'static, table form': dict(where=_plan, params=NOISY, T=T_STATIC, cap=63, table=True),       # 63: not a multiple of a block's 4 slots
    'static, drops': dict(where=_plan, params=PLAIN, T=T_STATIC, cap=26, drops=True),
    'sight': dict(where=_sight, params=WALLED, T=T_STATIC, cap=64, sight=True),
    'density, batch solver': dict(where=_plan, params=WALLED, T=T_DYNAMIC, cap=64, density=lambda: _density(every=8), updates=EVERY_8),
    'density + flow': dict(where=_plan, params=WALLED, T=T_DYNAMIC, cap=64, density=lambda: _density(every=8, flow=1.0),
                           updates=EVERY_8),
    'density, active solver': dict(where=_plan, params=WALLED, T=T_DYNAMIC, cap=64,
                                   density=lambda: _density(every=4, solver='active'), updates=EVERY_4),
    'density + exit choice': dict(where=_hall, params=WALLED, T=T_DYNAMIC, cap=64, density=lambda: _density(2.0, 0.5, every=8),
                                  updates=EVERY_8, choice=_choice),
}


def _retired_for_good(mask):
    """mask (S, T, cap) of the records -> the number of slots that were present, then absent for at least two recorded frames
    and to the end; asserts that no slot is present again after it retired (a slot holds one agent, ever)"""
    on = mask == 1
    again = np.zeros(on.shape[0::2], bool)
    gone = np.zeros_like(again)
    for t in range(1, on.shape[1]):
        gone |= on[:, t - 1] & ~on[:, t]
        again |= gone & on[:, t]
    assert not again.any()
    return int((on.any(1) & ~on[:, -2] & ~on[:, -1]).sum())


@pytest.mark.parametrize('form', list(FORMS))
def test_run_frame_by_frame_against_a_twin(form):
    from piml_amd.models.mlapm import MLAPM
    F = FORMS[form]
    (sc, base), params, T, cap = F['where'](), F['params'], F['T'], F['cap']
    density = F['density']() if 'density' in F else None
    choice = F['choice']() if 'choice' in F else None
    rep = TWIN.run(sc, base, params, T, cap, SEEDS, table=F.get('table', False), density=density, choice=choice)
    S, res, st = len(SEEDS), rep.result, rep.state
    c = rep.counts
    routed, left, branches = int(c[:, 0].sum()), int(c[:, 1].sum()), c[:, 2:6].sum(0).tolist()
    born, retired = c[:, 6:6 + S].sum(0).tolist(), c[:, 6 + S:].sum(0).tolist()
    share = left / max(routed, 1)
    mask = res.mask_p.cpu().numpy()
    for_good = _retired_for_good(mask)
    switches = None if rep.switches is None else rep.switches.sum(1).tolist()
    print(f'\n[mlapm routed] {form}: {T} frames, capacity {cap}: branches of the live rows {branches}; routed live rows {routed}, '
          f'left out (retired by the frame in A) {left} = {100 * share:.2f} %; born after frame 0 {born}, retired {retired}, '
          f'slots retired for good {for_good}, dropped {res.dropped}; updates at {rep.updates}; choices at {rep.choice_frames}, '
          f'switches {switches}, the fresh field decided at {rep.fresh_matters}; largest error of e against the host lookup '
          f'{rep.worst_e:.3g}')
    # every frame against its twin
    bad = np.argwhere(~rep.ok)
    assert bad.size == 0, (f'first difference at counter value {bad[0][0]}: {rep.names[bad[0][1]]}; in all '
                           f'{sorted({rep.names[j] for _, j in bad})}')
    assert share <= LEFT_OUT_CAP
    # a retired slot's records are record_retired's from then on, a never-filled one's the allocation's
    absent = torch.from_numpy(mask == 0).to(DEV)
    for t1 in range(T):
        assert bool((TWIN.retired_record(st, t1) | ~absent[:, t1]).all()), t1
    # nothing passed vacuously
    assert min(born) >= 1 and min(retired) >= 1 and for_good >= 1
    # (with the table branch 3 stands in front of branches 1 and 2 wherever a cell has a parent, which is every cell that is
    # routed at all: a run by the table shows branches 0 and 3 only, a run without it never shows branch 3)
    assert branches[0] >= 1 and (branches[3] >= 1) == bool(F.get('sight'))
    assert (branches[1] == 0 and branches[2] == 0) if F.get('sight') else branches[1] >= 1
    if F.get('drops'):
        assert min(res.dropped) > 0
    # the updates: when, and from which frame's crowd
    if density is not None:
        assert rep.updates == F['updates']
        for t, p, v, m in rep.snaps:
            assert torch.equal(bits(p), bits(res.position[:, t])) and torch.equal(bits(m), bits(res.mask_p[:, t])), t
            assert torch.equal(bits(v), bits(res.velocity[:, t])), t
    if choice is not None:
        assert rep.choice_frames == F['updates'] and max(switches) >= 1
    # the loop is the product loop, in all its paths
    kw = dict(capacity=cap, nav=base, nav_density=density, exit_choice=choice)
    sim = MLAPM(**params)
    runs = {'eager': sim.simulate_ensemble(sc, T, SEEDS, use_graph=False, **kw),
            'captured': sim.simulate_ensemble(sc, T, SEEDS, use_graph=True, frames_per_graph=8, **kw)}
    if F.get('table'):
        runs['sweep'] = MLAPM.simulate_sweep(sc, T, [params], SEEDS, **kw)
    for name, other in runs.items():
        for m in range(S):
            assert _same(res.member(m), other.member(m)), (name, m)
        if choice is not None:
            assert torch.equal(res.exit_switches, other.exit_switches), name


# ---- the update and the choice on one counter value: a crowd on which the fresh field decides ----

QUEUE = [(i, j) for j in range(2, 7) for i in range(9, 14)]      # (x, y) cells of the hall's grid: 25 agents before the near exit
NEAR_BOUND = [(26, 8), (25, 11), (23, 16), (22, 19)]             # probes bound for the near exit (gate 1)
FAR_BOUND = [(23, 10), (21, 14), (20, 17), (19, 19)]             # probes bound for the far exit (gate 2)
N_PLANTED = len(QUEUE) + len(NEAR_BOUND) + len(FAR_BOUND)


def _plant_the_queue(st):
    """Every agent of frame 0 (the scene has N_PLANTED of them) is moved by hand, to the centre of a cell of hall_field()'s
    grid.  Of each member's slots that came in through gate 0 -- for which both exits are candidates -- the first eight are
    the probes, placed about where the hall's two exits are equally far.  By the base field the far exit is the nearer one by
    1.4 to 1.8 cells at the near-bound probes -- less than the law's margin of 2 cells, so they stay -- and the near exit the
    nearer one by 2.4 to 2.9 cells at the far-bound probes -- more than the margin, so they switch.  The other 25 stand queued
    in front of the near exit, bound for gate 0, which is in no class.  With kd = 2, rho0 = 0.5 the queue (rho = 4 / m^2 in its
    window, f = 8) adds 1.3 to 2.7 cells to the near exit's plane at the probes, and still 0.6 to 1.9 with its first row gone
    (navcost_ref.deposit, cost and solve on these positions): the fresh field sends all eight to the far exit, the base field
    all eight to the near one.  -> the probes' slots, (S, 8)"""
    import scenario_ref
    from test_navchoice_gpu import HALL_BOUNDS, HALL_CELL
    ent = st.scenario.entries
    centre = lambda c: torch.tensor([HALL_BOUNDS[0] + (c[0] + 0.5) * HALL_CELL, HALL_BOUNDS[1] + (c[1] + 0.5) * HALL_CELL], device=DEV)
    mid = ent.shape[1] // 2
    assert bool((st.mask[:, :N_PLANTED] == 1).all()) and bool((st.mask[:, N_PLANTED:] == 0).all())
    probes = []
    for m, seed in enumerate(st.seed_list):
        oe = scenario_ref.agent_draws(seed, np.arange(N_PLANTED), ent.shape[0], ent.shape[1])['oe']
        slots = np.flatnonzero(oe == 0)[:len(NEAR_BOUND) + len(FAR_BOUND)].tolist()
        assert len(slots) == len(NEAR_BOUND) + len(FAR_BOUND), (seed, slots)
        rest = [i for i in range(N_PLANTED) if i not in slots]
        for i, c, g in ([(i, c, 1) for i, c in zip(slots, NEAR_BOUND)] + [(i, c, 2) for i, c in zip(slots[len(NEAR_BOUND):], FAR_BOUND)]
                        + [(i, c, 0) for i, c in zip(rest, QUEUE)]):
            st.p[m, i] = centre(c)
            st.exit_idx[m, :, i] = g
            st.waypoints[m, :, i] = ent[g, mid]
            st.dest[m, i] = ent[g, mid]
        probes.append(slots)
    st.p_res[:, 0], st.dest_res[:, 0] = st.p, st.dest            # the pair sources are read from the record
    return probes


def test_the_choice_reads_the_field_of_the_update_before_it(monkeypatch):
    """The hall with a crowd placed by hand after the init launch (_plant_the_queue), so that at counter value 1 -- the first
    update, with the base field before it -- the field of before the update and the fresh one choose differently for every
    probe.  The test's loop is checked as in the runs above (the choice against the restatement on the fresh field, the
    frames against their twins); here the restatement on the field of before the update must differ, the probes must be bound
    as the fresh field says, and the product loop, eager and captured, given the same crowd -- its init launch is followed
    by the same planting -- must end bitwise where the test's loop ends: a loop that chose before it updated would not."""
    from piml_amd import ops_scenario
    from piml_amd.models.mlapm import MLAPM
    from test_navchoice_gpu import hall, hall_field
    sc, base = hall(N_PLANTED, 2.0), hall_field()
    assert int(sc.n_initial) == N_PLANTED
    T, cap, density, choice = 18, 64, _density(2.0, 0.5, every=8), _choice()
    planted = []
    rep = TWIN.run(sc, base, WALLED, T, cap, SEEDS, density=density, choice=choice, plant=lambda st: planted.append(_plant_the_queue(st)))
    S, res = len(SEEDS), rep.result
    bad = np.argwhere(~rep.ok)
    assert bad.size == 0, f'first difference at counter value {bad[0][0]}: {rep.names[bad[0][1]]}'
    assert rep.updates == [1, 9] and rep.choice_frames == [1, 9]
    probes = np.array(planted[0])
    rows = np.arange(S)[:, None]
    fresh, stale = rep.chosen[1][:, 0][rows, probes], rep.stale[1][:, 0][rows, probes]
    switches = rep.switches.sum(1).tolist()
    print(f'\n[mlapm routed] planted queue: updates at {rep.updates}, choices at {rep.choice_frames}, the fresh field decided at '
          f'{rep.fresh_matters}; probes bound at counter value 1 by the fresh field {fresh.tolist()}, by the field before it '
          f'{stale.tolist()}; switches {switches}')
    assert 1 in rep.fresh_matters
    assert (fresh == 2).all() and (stale == 1).all()
    assert min(switches) >= len(NEAR_BOUND)
    # the product loop on the same crowd
    real = ops_scenario.scenario_step_mlapm

    def step_then_plant(st, law, *args, init=False, **kw):
        out = real(st, law, *args, init=init, **kw)
        if init:
            planted.append(_plant_the_queue(st))
        return out
    monkeypatch.setattr(ops_scenario, 'scenario_step_mlapm', step_then_plant)
    kw = dict(capacity=cap, nav=base, nav_density=density, exit_choice=choice)
    sim = MLAPM(**WALLED)
    for name, use_graph in (('eager', False), ('captured', True)):
        other = sim.simulate_ensemble(sc, T, SEEDS, use_graph=use_graph, frames_per_graph=8, **kw)
        assert len(planted) == 2 + use_graph and planted[-1] == planted[0], name
        for m in range(S):
            assert _same(res.member(m), other.member(m)), (name, m)
        assert torch.equal(res.exit_switches, other.exit_switches), name


# ---- planted edge rows ----

def _corner_cell(h):
    """(i, j, gate): a free cell beside a blocked corner at whose centre branch 2 applies and its rule -- a diagonal is skipped
    beside a cell that is not finite -- changes the neighbour"""
    blocked = h.blocked != 0
    near_wall = np.zeros_like(blocked)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near_wall[1:-1, 1:-1] |= blocked[1 + dy:blocked.shape[0] - 1 + dy, 1 + dx:blocked.shape[1] - 1 + dx]
    for j, i in zip(*np.nonzero(near_wall & ~blocked)):
        p = np.array([[h.x0 + (i + 0.5) * h.cell, h.y0 + (j + 0.5) * h.cell]], np.float32)
        for g in range(h.G):
            _, b, k = nav_ref.direction(h.u, h.x0, h.y0, h.cell, h.near, p, [g], p + 1)
            _, b0, k0 = nav_ref.direction(h.u, h.x0, h.y0, h.cell, h.near, p, [g], p + 1, skip_rule=False)
            if b[0] == 2 and b0[0] == 2 and k[0] != k0[0]:
                return int(i), int(j), g
    raise AssertionError('no cell where the corner rule binds')


@functools.lru_cache(maxsize=None)
def _plants():
    """the plan's field with a hand-made plateau in gate planes, and the planted rows (name, position, gate, the branch the
    static lookup must take there or None) of slots 0 .. len - 1"""
    from piml_amd import ops_scenario
    base = field('plan')
    u = base.u.clone()
    i0, j0 = 38, 28                                              # about (8, 6), in the open right room
    assert not base.blocked[j0 - 1:j0 + 3, i0 - 1:i0 + 3].any() and torch.isfinite(u[:, j0 - 1:j0 + 3, i0 - 1:i0 + 3]).all()
    for g in range(base.G):                                      # four equal centres, higher than every cell around them
        u[g, j0:j0 + 2, i0:i0 + 2] = u[g, j0:j0 + 2, i0:i0 + 2].max() + 1.0
    hand = ops_scenario.NavField(u, base.blocked, base.goal, base.x0, base.y0, base.cell, base.near, base.clearance)
    h = hand.to_numpy()
    x0, y0, c, gx, gy = h.x0, h.y0, h.cell, h.gx, h.gy
    centre = lambda i, j, fx=0.5, fy=0.5: (x0 + (i + fx) * c, y0 + (j + fy) * c)
    ci, cj, cg = _corner_cell(h)
    band = np.argwhere((h.blocked != 0) & ~(h.goal != 0).any(0))
    bj, bi = band[len(band) // 2]
    nj, ni = np.argwhere((h.u[1] > 0) & (h.u[1] <= h.near))[0]
    rows = [('outside, west', (x0 - 0.1, 3.0), 1, 0), ('outside, east', (x0 + gx * c + 0.1, 3.0), 0, 0),
            ('outside, south', (2.0, y0 - 0.1), 1, 0), ('outside, north', (2.0, y0 + gy * c + 0.1), 1, 0),
            ('blocked cell', centre(bi, bj), 1, 0),
            ('cell border', (x0 + 12 * c, y0 + 12.3 * c), 1, None),
            ('tile seam', (x0 + 32 * c, y0 + 32 * c), 0, None),
            ('last cell', centre(gx - 1, gy - 1), 0, 2),
            ('corner rule', centre(ci, cj), cg, 2),
            ('within near', centre(ni, nj), 1, 0),
            ('plateau', centre(i0, j0, 0.75, 0.75), 1, 2)]
    return hand, rows


@pytest.mark.parametrize('kind', ['static', 'sight', 'dynamic'])
def test_planted_edge_rows(kind):
    """after the init launch the first slots are moved by hand to where the lookup takes its other paths -- outside the grid on
    each side, inside a blocked cell, on a cell border, on the tile seam, in the grid's last cell, beside a blocked corner, within
    `near` of the gate, on a bilinear plateau -- one live slot gets flag 1 with another gate in row 0 of exit_idx, and one absent
    slot a finite position; then three twin frames, each with the host lookup of every live row"""
    from piml_amd import ops_scenario, scenarios
    sc = scene('plan')
    hand, rows = _plants()
    S, cap, T = len(SEEDS), 32, 4
    A = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=SEEDS)
    B = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=SEEDS)
    law, walls, noise = TWIN.laws(WALLED, A)
    ops_scenario.scenario_step_mlapm(A, None, init=True)
    n = len(rows)
    at = {name: i for i, (name, *_) in enumerate(rows)}
    ghost = 20
    assert bool((A.mask[:, :n + 1] == 1).all()) and bool((A.mask[:, ghost] == 0).all())      # the init launch filled slots 0 .. n
    ent = sc.entries
    for i, (_, p, g, _) in enumerate(rows):
        A.p[:, i] = torch.tensor(p, device=DEV)
        A.exit_idx[:, :, i] = g
        A.waypoints[:, :, i] = ent[g, ent.shape[1] // 2]
        A.dest[:, i] = ent[g, ent.shape[1] // 2]
    A.flag[:, n] = 1                                             # slot n: at its second waypoint, row 0 names the other gate
    A.exit_idx[:, 0, n] = 1 - A.exit_idx[:, 1, n]
    A.p[:, ghost] = torch.tensor([0.6, 1.1], device=DEV)         # an absent slot with a finite position: nobody counts it
    A.p_res[:, 0], A.dest_res[:, 0] = A.p, A.dest                # the pair sources are read from the record
    A.p_res[:, 0, ghost] = float('nan')
    nav = fields = {'static': hand, 'sight': sight_field(), 'dynamic': None}[kind]
    if kind == 'dynamic':
        density = _density(every=8)
        nav = ops_scenario.NavFieldDynamic(hand, S)
        nav.reset()                                              # as a run begins: the base in every member's planes
        snap = (A.p.clone(), A.v.clone(), A.mask.clone())
        ops_scenario.nav_field_update(nav, A, density)
        members = [0, S - 1]
        counted = TWIN.check_update(nav, TWIN.host_field(field('plan')), density, snap, members, 'planted update')
        # who deposits: the live slots inside the grid -- not the four planted outside it, not the ghost, which is inside
        p, live = snap[0][members].cpu().numpy(), snap[2][members].cpu().numpy() == 1
        c = np.floor((p - np.float32([hand.x0, hand.y0])) / np.float32(hand.cell))
        inside = (c[..., 0] >= 0) & (c[..., 0] < hand.gx) & (c[..., 1] >= 0) & (c[..., 1] < hand.gy)
        assert inside[:, ghost].all() and not live[:, ghost].any()
        assert (live & ~inside).sum(1).tolist() == [sum(name.startswith('outside') for name in at)] * len(members)
        assert counted == int((live & inside).sum())
        fields = [nav.member(m) for m in range(S)]

    def step(st, routed):
        ops_scenario.scenario_step_mlapm(st, law, walls=walls, noise=noise, nav=nav if routed else None)
    oks, seen_branches = [], set()
    for t in range(T - 1):
        ok, counts, seen = TWIN.twin_frame(A, B, fields, step, t)
        oks.append(ok)
        TWIN.check_lookup(seen, fields, f'{kind}, frame {t}')
        b = seen[4].cpu().numpy()
        seen_branches |= set(b[seen[6].cpu().numpy()].tolist())
        if t == 0:
            print(f'\n[mlapm routed] planted rows, {kind}: branches ' + ', '.join(f'{name} {b[:, i].tolist()}' for i, (name, *_)
                                                                                   in enumerate(rows)) + f', flag 1 {b[:, n].tolist()}')
            if kind == 'static':
                for i, (name, _, _, want) in enumerate(rows):
                    assert want is None or (b[:, i] == want).all(), (name, b[:, i], want)
            if kind != 'sight':
                assert (b[:, at['last cell']] == 2).all() and (b[:, at['corner rule']] == 2).all()           # descent
            assert (b[:, n] > 0).all()                           # the flag-1 slot is routed, by the gate of row 1
    bad = np.argwhere(~torch.stack(oks).cpu().numpy())
    assert bad.size == 0, f'first difference at counter value {bad[0][0]}: {TWIN.FRAME_CHECKS[bad[0][1]]}'
    assert 2 in seen_branches or kind == 'sight'
