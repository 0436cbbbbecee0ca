"""A routed MLAPM run driven by the test itself, frame by frame against a twin (test_scenario_mlapm_routed_gpu.py).

run() follows the schedule MLAPM._run_scenario's docstring states -- the init launch, the noise state and the switch counter,
then for every counter value t = 0 .. T-2 the field update when t >= 1 and (t - 1) % every == 0, the exit choice in front of
the frame, the frame -- with the public primitives of ops_scenario, and checks as it goes:

  the frame   state A is copied into a twin B, B's destination is overwritten by where(b > 0, p + e, dest) of
              ops_scenario.nav_direction on B's state, A steps with the field and B without it (twin_frame);
  the lookup  on a stride of frames (e, branch, neighbour) against nav_ref / navsight_ref on the host;
  the update  nav_field_update's count, momentum, cost and field of members 0 and the last against navcost_ref / navflow_ref
              (/ navactive_ref for the work) on the positions the run itself handed it;
  the choice  nav_choose_exit against navchoice_ref.choose on the state and the field the member reads at that moment.

The device comparisons are collected as booleans on the device and read once, at the end of the run."""
import types

import numpy as np
import torch

import nav_ref
import navactive_ref
import navcost_ref
import navflow_ref
import navsight_ref
from test_scenario_mlapm_gpu import bits
from test_scenario_routed_gpu import STATE

DEV = 'cuda:0'
SLOT = ('p', 'v', 'a', 'dest', 'flag', 'mask', 'desired_speed', 'hist')         # (S, cap[, k])
WAY = ('waypoints', 'exit_idx')                                                  # (S, D, cap[, 2])
REC = ('p_res', 'v_res', 'a_res', 'dest_res', 'mask_res')                        # (S, T, cap[, 2]): the record of t + 1
WHOLE = ('spawned', 'spawn_count', 'dropped')
PER_SLOT = SLOT + WAY + REC
assert set(PER_SLOT + WHOLE) == set(STATE)
COPIED = STATE + ('selff', 'spawn_iters')                                        # everything a frame may read
KEPT = ('p', 'v', 'a', 'hist', 'p_res', 'v_res', 'a_res', 'mask_res')            # what an arrival at a waypoint leaves alone
E_TOL = 1e-5                                                                     # the lookup tests' (hardware rsq)


def u32(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


def copy_state(A, B):
    """everything the frame reads: the state tensors and records, the frame counter, the noise state"""
    from piml_amd import ops_scenario
    for k in COPIED:
        getattr(B, k).copy_(getattr(A, k))
    B.t.copy_(A.t)
    if A.noise_state is not None:
        ops_scenario.scenario_noise_state(B).copy_(A.noise_state)


def gate_of(st):
    """exit_idx[flag] of every slot (a retired slot's flag may be D: clamped, the lookup leaves its NaN row in branch 0)"""
    D = st.exit_idx.shape[-2]
    return torch.gather(st.exit_idx, -2, st.flag.clamp(max=D - 1).long().unsqueeze(-2)).squeeze(-2)


def directions(st, fields):
    """(e, branch, neighbour) of ops_scenario.nav_direction on st's state; fields: the scene's NavField, or one per member"""
    from piml_amd import ops_scenario
    gate = gate_of(st)
    if not isinstance(fields, (list, tuple)):
        return ops_scenario.nav_direction(st.p, gate, st.dest, fields, return_branch=True)
    out = [ops_scenario.nav_direction(st.p[m], gate[m], st.dest[m], f, return_branch=True) for m, f in enumerate(fields)]
    return tuple(torch.stack(x) for x in zip(*out))


def laws(params, st, table=False):
    """(law, walls, noise) of scenario_step_mlapm for MLAPM(**params); table: the per-member table forms with one row each"""
    from piml_amd import ops_scenario
    from piml_amd.models import mlapm
    S, dt = st.seeds.numel(), float(st.scenario.time_unit)
    law = mlapm.MLAPM(**params)._law(0.3)
    wall, noise = mlapm.wall_args(params), mlapm.noise_args(params)
    walls = None if wall is None else (ops_scenario.wall_grid(st.scenario.obstacles, wall[2], DEV), ops_scenario.wall_law(*wall[:2]))
    noise = None if noise is None else ops_scenario.noise_law(*noise, dt)
    if table:
        law = ops_scenario.mlapm_law_table([law] * S, DEV)
        if walls is not None:
            walls = (walls[0], ops_scenario.wall_law_table([walls[1]] * S, DEV))
        if noise is not None:
            noise = ops_scenario.noise_law_table([noise] * S, dt, DEV)
    return law, walls, noise


def _rows(st, k, t1):
    """tensor k of st as (S, cap, -1) bit patterns: the state rows, the waypoint rows, or the record of frame t1"""
    x = bits(getattr(st, k))
    if k in WAY:
        x = x.transpose(1, 2)
    elif k in REC:
        x = x[:, t1]
    return x.reshape(x.shape[0], x.shape[1], -1)


def retired_record(st, t1):
    """(S, cap) bool: frame t1's record of the slot is what record_retired writes -- NaN position and destination, zero
    velocity, acceleration and mask"""
    return (st.p_res[:, t1].isnan().all(-1) & st.dest_res[:, t1].isnan().all(-1) & (bits(st.v_res[:, t1]) == 0).all(-1)
            & (bits(st.a_res[:, t1]) == 0).all(-1) & (bits(st.mask_res[:, t1]) == 0))


FRAME_CHECKS = tuple(f'kept:{k}' for k in KEPT) + tuple(f'straight:{k}' for k in PER_SLOT) + \
    tuple(f'not live:{k}' for k in PER_SLOT) + WHOLE + ('noise state', 'B retires only whom A retires', 'left out: retired record')


def twin_frame(A, B, fields, step, t):
    """One frame at counter value t.  B becomes A's copy with dest = where(b > 0, p + e, dest) of the lookup on its own state
    through `fields`, in the present slots (the frame steps no other); step(st, routed) runs the frame on st, with the field
    (A) or without (B).  -> (ok (len(FRAME_CHECKS)) bool, counts (2 + 4 + 2 S) int64: routed live rows, of them left out, the
    branch histogram of the live rows, the rows born and the rows retired in A per member, the lookup (P, gate, dest, e, b,
    nb, live) of before the frame) on the device"""
    copy_state(A, B)
    e, b, nb = directions(B, fields)
    seen = (B.p.clone(), gate_of(B), B.dest.clone(), e, b, nb)
    live = A.mask == 1                                           # (an absent slot has a NaN position and b = 0 -- unless planted)
    B.dest.copy_(torch.where(((b > 0) & live).unsqueeze(-1), B.p + e, B.dest))
    step(A, True)
    step(B, False)
    t1 = t + 1
    gone_a, gone_b = live & (A.mask == 0), live & (B.mask == 0)
    kept, straight, left = live & ~gone_a & ~gone_b, live & (b == 0), live & (b > 0) & gone_a

    def same(k, rows):
        return ((_rows(A, k, t1) == _rows(B, k, t1)).all(-1) | ~rows).all()
    ok = [same(k, kept) for k in KEPT] + [same(k, straight) for k in PER_SLOT] + [same(k, ~live) for k in PER_SLOT]
    ok += [(bits(getattr(A, k)) == bits(getattr(B, k))).all() for k in WHOLE]
    ok.append(torch.tensor(True, device=DEV) if A.noise_state is None else (bits(A.noise_state) == bits(B.noise_state)).all())
    ok.append((~gone_b | gone_a).all())
    ok.append((~left | ((A.mask == 0) & A.p.isnan().all(-1) & retired_record(A, t1))).all())
    counts = torch.cat([torch.stack([(live & (b > 0)).sum(), left.sum()]), torch.bincount(b[live].long(), minlength=4)[:4],
                        (~live & (A.mask == 1)).sum(1), gone_a.sum(1)])
    return torch.stack(ok), counts, seen + (live,)


def check_lookup(seen, fields, what=''):
    """the device lookup of the live rows against the host restatement: branch and neighbour exactly, e to E_TOL.  fields: as
    directions takes them.  -> the largest error of e"""
    P, gate, dest, e, b, nb, live = (x.cpu().numpy() for x in seen)
    worst = 0.0
    for m in range(P.shape[0]):
        f = fields[m] if isinstance(fields, (list, tuple)) else fields
        rows = np.flatnonzero(live[m])
        if rows.size == 0:
            continue
        u = f.u.cpu().numpy()
        args = (f.x0, f.y0, f.cell, f.near, P[m][rows], gate[m][rows], dest[m][rows])
        if f.sight_desc is not None:
            e_want, b_want, k_want = navsight_ref.direction(u, f.parent.cpu().numpy(), *args)
        else:
            e_want, b_want, k_want = nav_ref.direction(u, *args)
        assert np.array_equal(b[m][rows], b_want), (what, m, rows[b[m][rows] != b_want][:8])
        assert np.array_equal(nb[m][rows], k_want), (what, m, rows[nb[m][rows] != k_want][:8])
        fin = np.isfinite(e_want).all(1)
        assert np.array_equal(np.isfinite(e[m][rows]).all(1), fin), (what, m)
        if fin.any():
            worst = max(worst, float(np.abs(e[m][rows][fin] - e_want[fin]).max()))
    assert worst <= E_TOL, (what, worst)
    return worst


def check_update(dyn, host, law, snap, members, what=''):
    """nav_field_update's product for `members` against the restatements on the snapshot (p, v, mask) it was handed: the
    count (and momentum), the cost plane(s), the solved field, and under solver='active' the stalled word and the tiles
    stepped.  host: the base field's numpy namespace (with descent for a flow law)"""
    P, V, M = (x[members].cpu().numpy() for x in snap)
    r = law.radius_cells(dyn.cell)
    grid = (dyn.x0, dyn.y0, dyn.cell, dyn.gx, dyn.gy)
    if law.flow > 0:
        count, mom = navflow_ref.deposit_flow(P, V, M, *grid)
        f = navflow_ref.cost_flow(count, mom, host.descent, dyn.cell, r, law.kd, law.rho0, law.fmax, law.flow, law.vref)
        u = np.stack([navflow_ref.solve_gates(host.blocked, host.goal, f[j])[0] for j in range(len(members))])
        assert np.array_equal(dyn.mom[members].cpu().numpy(), mom), (what, 'mom')
        cost = dyn.cost_gates
    else:
        count = navcost_ref.deposit(P, M, *grid)
        f, _ = navcost_ref.cost(count, dyn.cell, r, law.kd, law.rho0, law.fmax)
        u = np.stack([navcost_ref.solve(host.blocked, host.goal, f[j])[0] for j in range(len(members))])
        cost = dyn.cost
    assert np.array_equal(dyn.count[members].cpu().numpy(), count), (what, 'count')
    assert np.array_equal(u32(cost[members]), u32(f)), (what, 'cost')
    assert np.array_equal(u32(dyn.u[members]), u32(u)), (what, 'u', int((u32(dyn.u[members]) != u32(u)).sum()))
    if law.solver == 'active':
        assert int(dyn.stalled.item()) == 0, (what, 'stalled')
        ref = navactive_ref.relax_active(host.blocked, host.goal, f, launches=dyn.max_launches)
        assert not ref.stalled and np.array_equal(u32(ref.u), u32(u)), (what, 'the restated active solve')
        assert np.array_equal(dyn.work.view(dyn.members, dyn.G)[members].cpu().numpy(), ref.work), (what, 'work')
    return int(count.sum())


def host_field(base, flow=False):
    h = base.to_numpy()
    if flow:
        h.descent = navflow_ref.descent_dir(h.u)
    return h


def run(sc, base, params, T, cap, seeds, table=False, density=None, choice=None, stride=8, plant=None):
    """The run (see the module's docstring).  base: the scene's static NavField, with or without the any-angle table; density:
    None or a nav_density_law (a NavFieldDynamic over base is made here); choice: None or an exit_choice_law; plant: None or a
    function of the state, called once after the init launch (a test moves the agents of frame 0 by hand with it).  Host-side
    comparisons assert here; the device-side ones come back in the report: result (scenario_result of the loop's state), ok
    (T - 1, len(names)) bool, names, counts (T - 1, 6 + 2 S), updates (the counter values an update ran at), snaps (its
    (t, p, v, mask) snapshots), switches (S, cap) or None, choice_frames (the counter values a choice was scheduled at),
    fresh_matters (of them, those where the field of before the update would have chosen otherwise), chosen and stale (per
    counter value of fresh_matters' candidates -- a choice and an update together -- exit_idx (S, D, cap) of the restatement on
    the fresh field, which the device agreed with, and on the field of before the update), worst_e, state, dyn"""
    from piml_amd import ops_scenario, scenarios
    S = len(seeds)
    A = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=seeds)
    B = scenarios.scenario_state_for(sc, T, cap, DEV, seeds=seeds)
    law, walls, noise = laws(params, A, table)
    dyn, nav, fields, members = None, base, base, sorted({0, S - 1})
    if density is not None:
        dyn = ops_scenario.NavFieldDynamic(base, S, flow=density.flow > 0)
        dyn.reset()
        nav, host = dyn, host_field(base, density.flow > 0)
        per_member = [dyn.member(m) for m in range(S)]           # views of dyn.u: they follow the updates
        still = dyn.u.clone()
        assert np.array_equal(u32(dyn.u), u32(base.u.unsqueeze(0).expand_as(dyn.u)))      # the static base before any update
    ops_scenario.scenario_step_mlapm(A, None, init=True)
    if plant is not None:
        plant(A)
    if noise is not None:
        ops_scenario.scenario_noise_state(A)
    if choice is not None:
        ops_scenario.scenario_exit_switches(A)
        # the restatement of a choice pass on a state as it stands is test_navchoice_gpu.py's own (_restate: navchoice_ref.choose
        # per member on the host copies of st.p, dest, flag, mask, waypoints, exit_idx and spawned, with st.seed_list, st.members
        # and st.scenario), and WRITTEN its list of what a pass may write
        from test_navchoice_gpu import WRITTEN, _restate
        choice_state = tuple(k for k in COPIED if k not in WRITTEN)

    def step(st, routed):
        ops_scenario.scenario_step_mlapm(st, law, walls=walls, noise=noise, nav=nav if routed else None)
    ok, counts, updates, snaps, choice_frames, fresh_matters, worst_e = [], [], [], [], [], [], 0.0
    chosen, stale_chosen = {}, {}
    for t in range(T - 1):
        extra = []
        # 1. the field update, before the frame at counter value t
        before_update = None
        if density is not None:
            if t >= 1 and (t - 1) % density.every == 0:
                snap = (A.p.clone(), A.v.clone(), A.mask.clone())
                before_update = types.SimpleNamespace(u=dyn.u.clone(), x0=dyn.x0, y0=dyn.y0, cell=dyn.cell)
                ops_scenario.nav_field_update(dyn, A, density)
                check_update(dyn, host, density, snap, members, f'update at {t}')
                updates.append(t)
                snaps.append((t,) + snap)
                still = dyn.u.clone()
                fields = per_member
            else:
                extra.append((bits(dyn.u) == bits(still)).all())  # between updates the field does not change
        # 2. the exit choice, in front of the frame
        if choice is not None:
            before = {k: getattr(A, k).clone() for k in COPIED + ('exit_switches',)}
            scheduled = t >= 1 and (t - 1) % choice.every == 0
            if scheduled:
                want, switched = _restate(A, nav, choice, t)
            ops_scenario.nav_choose_exit(A, nav, choice, A.exit_switches)
            if scheduled:
                choice_frames.append(t)
                for k in WRITTEN:
                    ref = torch.from_numpy(np.stack([s[k] for s in want])).to(DEV)
                    assert torch.equal(bits(getattr(A, k)), bits(ref)), (f'choice at {t}', k)
                for k in choice_state:
                    assert torch.equal(bits(getattr(A, k)), bits(before[k])), (f'choice at {t}', k)
                assert torch.equal(A.exit_switches, before['exit_switches'] + torch.from_numpy(switched).to(DEV)), f'choice at {t}'
                if before_update is not None:                    # an update fell on this counter value: the choice read the fresh field
                    # (the state of before the choice for _restate: A's attributes -- plain instance attributes, seeds and
                    # scenario among them -- with the tensors of the snapshot in place of the ones the launch has written)
                    stale, _ = _restate(types.SimpleNamespace(**{**vars(A), **before}), before_update, choice, t)
                    chosen[t] = np.stack([s['exit_idx'] for s in want])
                    stale_chosen[t] = np.stack([s['exit_idx'] for s in stale])
                    if any(not np.array_equal(u32(a[k]), u32(b[k])) for a, b in zip(stale, want) for k in WRITTEN):
                        fresh_matters.append(t)
            else:                                                # an unscheduled launch leaves everything alone
                extra.append(torch.stack([(bits(getattr(A, k)) == bits(v)).all() for k, v in before.items()]).all())
        # 3. the frame, against its twin
        o, c, seen = twin_frame(A, B, fields, step, t)
        while len(extra) < 2:
            extra.append(torch.tensor(True, device=DEV))
        ok.append(torch.cat([o, torch.stack(extra)]))
        counts.append(c)
        if t % stride == 0 or t == T - 2:
            worst_e = max(worst_e, check_lookup(seen, fields, f'lookup at {t}'))
    torch.cuda.synchronize()
    assert int(A.t.item()) == T - 1
    if density is not None and density.solver == 'active':
        dyn.check_converged()
    return types.SimpleNamespace(
        result=scenarios.scenario_result(A), ok=torch.stack(ok).cpu().numpy(), names=FRAME_CHECKS + ('extra 0', 'extra 1'),
        counts=torch.stack(counts).cpu().numpy(), updates=updates, snaps=snaps, choice_frames=choice_frames,
        fresh_matters=fresh_matters, chosen=chosen, stale=stale_chosen, switches=None if choice is None else A.exit_switches, worst_e=worst_e, state=A, dyn=dyn)
