"""The inputs of test_rollout_step_gpu.py and what test_rollout_step_ref.py checks of them without a GPU: rollout states for
the inference step kernel (piml_rollout_step / piml_rollout_step_ksum, piml_amd/csrc/pairwise.hip) outside what
tests/golden/rollout.npz reaches -- several waypoints per agent, velocity histories of two and three frames, slices with
their own and with shared waypoints, a last workgroup with 255 / 256 / 257 / 258 rows, a start above frame 0.

A case is built from SEEDS: `case(name)` -> (data, a_table, t_start).  `data` has the fields BaseSimulator._rollout_state
reads (position, velocity, acceleration, destination (*c, T, N, 2), dest_idx (*c, T, N), dest_num (N), waypoints
(*c, D, N, 2) or (D, N, 2), self_features (*c, T, N, 2 H + 5), ped_features, obs_features, obstacles, mask_p,
mask_p_pred (*c, T, N), num_frames, time_unit); `a_table` (*c, T, N, 2) stands in for the network's output of each frame.

Agents walk along a line of waypoints about 1 m apart at 2-3 m/s (0.16-0.24 m a frame), so switches and arrivals fall
inside the window.  The time series is the walk itself (no agent leaves it), absent frames are NaN positions.  Agents
placed by hand where N >= 9 (ROLES), in every slice:
  0  position - destination exactly (0.5, 0) at frame 0: the switch is a strict <, no switch
  1  (nextafter(0.5, 0), 0): switches
  2  (0, 0.5): no switch
  3  one waypoint; re-enters (mask_p - mask_p_pred = 1) in the frame after the one in which it arrives: the injection wins
  4  never present: NaN position, velocity and acceleration in every frame, and a NaN in a_table
  5  enters at frame 1, NaN velocity and history before
  6  enters at frame T - 1
  7  one waypoint
The others enter late with probability 0.3 and have 1..D waypoints."""
import functools
import types

import numpy as np
import torch

import rollout_step_ref as R

DT = 0.08
KP, KO, N_OBS = 3, 2, 5                      # neighbour slots of the feature buffers the driver runs fill
MARGIN = 1e-4                                # no | |p - dest| - 0.5 | below this outside the hand-placed points
SEEDS = dict(multi_wp=301, hist3=302, hist2=305, slices=304, tails=306)
SPECS = dict(
    multi_wp=dict(C=None, T=12, N=40, D=3, H=1),
    hist3=dict(C=None, T=12, N=40, D=3, H=3),
    hist2=dict(C=None, T=6, N=9, D=3, H=2, gap=0.6),
    slices=dict(C=3, T=12, N=40, D=3, H=1),
    shared_wp=dict(C=3, T=12, N=40, D=3, H=1),
    late_start=dict(C=None, T=12, N=40, D=3, H=1, t_start=3),
    tails_255=dict(C=None, T=4, N=255, D=2, H=1),
    tails_256=dict(C=None, T=4, N=256, D=2, H=1),
    tails_257=dict(C=1, T=4, N=257, D=2, H=1),
    tails_3x86=dict(C=3, T=4, N=86, D=2, H=1),
    tails_1=dict(C=None, T=4, N=1, D=2, H=1),
)
REFERENCE = ('multi_wp', 'hist3', 'hist2', 'slices', 'late_start')      # what the reference can run and the .npz records
RESTATED = ('shared_wp', 'tails_255', 'tails_256', 'tails_257', 'tails_3x86', 'tails_1')
ALL = REFERENCE + RESTATED
MIN_EVENTS = dict(advances=6, arrivals=3, entries=3, arrive_and_enter=1)
ROLES = dict(exact_x=0, below_x=1, exact_y=2, arrive_enter=3, never=4, enter_1=5, enter_last=6, one_wp=7)


def _scene(g, geometry_seed, T, N, D, H, dest_num, enter, gap, moved):
    """one slice: the walk of N agents as a time series.  The slices of a case share starts, headings and speeds
    (`geometry_seed`); a slice after the first has its waypoints moved by 0.15 m (`moved`) and its own entry frames."""
    f32 = torch.float32
    gg = torch.Generator().manual_seed(geometry_seed)
    ang = 2 * np.pi * torch.rand(N, generator=gg, dtype=torch.float64)
    u = torch.stack((torch.cos(ang), torch.sin(ang)), -1)                       # heading
    speed = 2 + torch.rand(N, generator=gg, dtype=torch.float64)               # 2..3 m/s
    start = 20 * torch.rand(N, 2, generator=gg, dtype=torch.float64)
    first = 0.55 + 0.6 * torch.rand(N, generator=gg, dtype=torch.float64)      # distance to the first waypoint
    along = first.unsqueeze(0) + gap * torch.arange(D, dtype=torch.float64).unsqueeze(1) \
        + 0.1 * torch.randn(D, N, generator=gg, dtype=torch.float64)
    wp = start.unsqueeze(0) + along.unsqueeze(-1) * u.unsqueeze(0) + 0.05 * torch.randn(D, N, 2, generator=gg, dtype=torch.float64)
    if moved:
        wp = wp + 0.15 * torch.randn(D, N, 2, generator=g, dtype=torch.float64)
    wp = wp.to(f32)
    roles = N >= 9
    if roles:
        r = ROLES
        half = float(np.nextafter(np.float32(0.5), np.float32(0)))
        for i, (dx, dy) in ((r['exact_x'], (0.5, 0.0)), (r['below_x'], (half, 0.0)), (r['exact_y'], (0.0, 0.5))):
            # the first waypoint at the origin, the start at the offset: position - destination is the offset exactly
            wp[:, i] = wp[:, i] - wp[0, i]
            start[i] = torch.tensor([dx, dy], dtype=torch.float64)
            d = -start[i] / start[i].norm()
            u[i] = d
            wp[1:, i] = (torch.arange(1, D, dtype=torch.float64).unsqueeze(-1) * gap * d).to(f32)
        start[r['arrive_enter']] = wp[0, r['arrive_enter']].double() - 0.75 * u[r['arrive_enter']]

    v_walk = speed.unsqueeze(-1) * u
    pos = torch.full((T, N, 2), float('nan'), dtype=f32)
    vel = torch.zeros(T, N, 2, dtype=f32)
    acc = torch.zeros(T, N, 2, dtype=f32)
    idx = torch.zeros(T, N, dtype=torch.long)
    p = start.to(f32)
    if roles:                                     # the exact offsets survive the float32 conversion
        assert float(p[ROLES['below_x'], 0]) == half
    cur = torch.zeros(N, dtype=torch.long)
    jit_v = 0.05 * torch.randn(T, N, 2, generator=g, dtype=torch.float64)
    jit_a = 0.3 * torch.randn(T, N, 2, generator=g, dtype=torch.float64)
    for t in range(T):
        here = t >= enter
        pos[t, here] = p[here]
        vel[t, here] = (v_walk + jit_v[t]).to(f32)[here]
        acc[t, here] = jit_a[t].to(f32)[here]
        idx[t] = cur
        d = torch.gather(wp, 0, cur.view(1, N, 1).expand(1, N, 2))[0]
        near = ((p - d).norm(dim=-1) < 0.5) & (cur < dest_num - 1)
        cur = cur + near.long()
        p = (p.double() + v_walk * DT).to(f32)
    dest = torch.gather(wp, 0, idx.unsqueeze(-1).expand(T, N, 2))
    hist = vel.unsqueeze(-2) + 0.1 * torch.randn(T, N, H, 2, generator=g).to(f32)         # H earlier velocities, any values
    if roles:
        for i in (ROLES['never'], ROLES['enter_1']):
            absent = torch.arange(T) < enter[i]
            vel[absent, i] = float('nan')
            hist[absent, i] = float('nan')
        acc[:, ROLES['never']] = float('nan')
    rel = torch.nan_to_num(dest - pos, nan=0.0)
    selff = torch.cat((rel, hist.reshape(T, N, 2 * H), acc, speed.to(f32).view(1, N, 1).expand(T, N, 1)), -1)
    dest = torch.where(pos.isnan(), pos, dest)                                   # an absent agent's destination is NaN too
    mask = (torch.arange(T).unsqueeze(-1) >= enter.unsqueeze(0)).to(f32)
    pred = mask.clone()
    late = (enter > 0) & (enter < T)
    pred[enter[late], torch.nonzero(late).squeeze(-1)] = 0                       # the entry frame: mask_p - mask_p_pred = 1
    return dict(position=pos, velocity=vel, acceleration=acc, destination=dest, dest_idx=idx, waypoints=wp,
                self_features=selff.contiguous(), mask_p=mask, mask_p_pred=pred)


def _build(name):
    base = {'shared_wp': 'slices', 'late_start': 'multi_wp'}.get(name, name)
    spec = SPECS[base]
    seed = SEEDS['tails'] + spec['N'] if base.startswith('tails') else SEEDS[base]
    g = torch.Generator().manual_seed(seed)
    C, T, N, D, H = (spec[k] for k in 'CTNDH')
    gap = spec.get('gap', 1.0)
    t_start = SPECS[name].get('t_start', 0)
    dest_num = torch.randint(1, D + 1, (N,), generator=g)
    if N >= 9:
        for k in ('exact_x', 'below_x', 'exact_y'):
            dest_num[ROLES[k]] = D
        dest_num[ROLES['arrive_enter']] = 1
        dest_num[ROLES['one_wp']] = 1
    slices = []
    for c in range(C or 1):
        enter = torch.where(torch.rand(N, generator=g) < 0.3, torch.randint(2, max(T - 1, 3), (N,), generator=g), 0)
        if N >= 9:
            for k in ('exact_x', 'below_x', 'exact_y', 'arrive_enter', 'one_wp'):
                enter[ROLES[k]] = 0
            enter[ROLES['never']] = T
            enter[ROLES['enter_1']] = 1
            enter[ROLES['enter_last']] = T - 1
        slices.append(_scene(g, seed + 1000, T, N, D, H, dest_num, enter, gap, moved=c > 0))
    data = types.SimpleNamespace()
    for k in slices[0]:
        data.__dict__[k] = slices[0][k] if C is None else torch.stack([s[k] for s in slices])
    data.dest_num = dest_num
    data.num_frames, data.time_unit, data.meta_data = T, DT, None
    lead = () if C is None else (C,)
    data.ped_features = torch.zeros(*lead, T, N, KP, 6)
    data.obs_features = torch.zeros(*lead, T, N, KO, 6)
    data.obstacles = 20 * torch.rand(N_OBS, 2, generator=g)
    a_table = 0.5 * torch.randn(*lead, T, N, 2, generator=g)
    if N >= 9:
        a_table[..., 2, ROLES['never'], :] = float('nan')
        a_table[..., T - 2, ROLES['never'], :] = float('nan')
    if name == 'shared_wp':
        data.waypoints = data.waypoints[0].clone()
    return data, a_table, t_start


@functools.lru_cache(maxsize=None)
def _case(name):
    data, a_table, t_start = _build(name)
    if data.position.shape[-2] >= 9:
        # agent 3 re-enters in the frame after the one in which it arrives: the frame is read off a run without the flag
        # (nothing before the flag's frame depends on it)
        i = ROLES['arrive_enter']
        _, rec = R.run(R.series(data), a_table.numpy(), t_start)
        gone = np.stack([r.events.gone[..., i] for r in rec], axis=-1)          # (*c, frames)
        for c, row in enumerate(gone.reshape(-1, gone.shape[-1])):
            k = t_start + int(np.argmax(row))
            assert row.any() and k + 1 < data.num_frames, (name, c, row)
            pred = data.mask_p_pred if data.position.dim() == 3 else data.mask_p_pred[c]
            pred[k + 1, i] = 0
    return data, a_table, t_start


def case(name):
    """(data, a_table, t_start) of a case: fresh copies, the callee may write them"""
    data, a_table, t_start = _case(name)
    return clone(data), a_table.clone(), t_start


def clone(data):
    """a copy whose tensors the callee may write"""
    out = types.SimpleNamespace()
    for k, v in data.__dict__.items():
        out.__dict__[k] = v.clone() if isinstance(v, torch.Tensor) else v
    return out


@functools.lru_cache(maxsize=None)
def restated(name, remove_arrived=True):
    """the restatement's run of a case: (final state, per-frame records) of rollout_step_ref.run.  Read only."""
    data, a_table, t_start = _case(name)
    return R.run(R.series(data), a_table.numpy(), t_start, remove_arrived)


def events(name):
    """what the restated run of a case contains: index advances, arrivals, entries, frames in which an agent arrives and
    enters at once, and the smallest | |p - dest| - 0.5 | (float64) outside the three hand-placed points"""
    data, _, t_start = _case(name)
    _, rec = restated(name)
    count = dict(advances=0, arrivals=0, entries=0, arrive_and_enter=0)
    margin = np.inf
    for k, r in enumerate(rec):
        e = r.events
        count['advances'] += int((e.near & ~e.gone).sum())
        count['arrivals'] += int(e.gone.sum())
        count['entries'] += int(e.enter.sum())
        count['arrive_and_enter'] += int((e.enter & e.gone).sum())
        off = np.abs(e.dist - 0.5)
        if k == 0 and t_start == 0 and off.shape[-1] >= 9:
            hand = [ROLES[x] for x in ('exact_x', 'below_x', 'exact_y')]
            assert np.all(off[..., hand] < 1e-7), name                         # they are where they were put
            off[..., hand] = np.inf
        margin = min(margin, float(np.nanmin(off)))
    count['margin'] = margin
    return count
