"""Open-world scenario operators over the C ABI (include/piml_hip.h: piml_scenario_step, piml_scenario_step_rules,
piml_scenario_step_members, piml_scenario_step_mlapm, piml_scenario_step_mlapm_laws, piml_scenario_route).

`scenario_state` allocates the persistent (static-address) buffers of one simulation or an ensemble and the
`piml_scenario` descriptor that points at them; `scenario_step` is one launch per simulated frame (integrate, arrive,
retire, spawn, record), with the frame index read from device memory so that one captured launch serves every frame of a
replayed graph.  Like every operator of piml_amd they require GPU tensors and raise PimlHipError otherwise."""
import ctypes
import math
import types

import torch

from . import _lib
from .ops import _gpu_f32, _ptr, _stream

MAX_MEMBERS = 65535          # piml_scenario_step_members: one grid row per member


def scenario_route(origin, destination, polyline, max_iters=16, clearance=2.0):
    """utils.route (src/utils/utils.py:141-165) for every (origin, destination) pair, one wave each: (n, 2) x2, polyline
    (R, 2) -> (waypoint r (n, 2), iterations (n) int32).  The route of pair j is (origin[j], r[j], destination[j])."""
    o = _gpu_f32('origin', origin).reshape(-1, 2)
    d = _gpu_f32('destination', destination).reshape(-1, 2)
    poly = _gpu_f32('polyline', polyline).reshape(-1, 2)
    if o.shape != d.shape:
        raise ValueError(f'origin {tuple(o.shape)} and destination {tuple(d.shape)} differ')
    if o.device != d.device or o.device != poly.device:
        raise ValueError('origin, destination and polyline on different devices')
    r = torch.empty_like(o)
    iters = torch.empty(o.shape[0], device=o.device, dtype=torch.int32)
    with torch.cuda.device(o.device):
        _lib.check(_lib.lib().piml_scenario_route(_ptr(o), _ptr(d), o.shape[0], _ptr(poly), poly.shape[0], int(max_iters),
                                                  float(clearance), _ptr(r), _ptr(iters), _stream()), 'piml_scenario_route')
    return r, iters


def scenario_state(scenario, capacity, frames, hist_width=2, seed=0, topk_ped=6, topk_obs=10, seeds=None):
    """The buffers of one simulation of `scenario` (on its device) with `capacity` slots and `frames` recorded frames,
    and their descriptor.  Absent slots start as NaN positions / destinations, zero velocity, acceleration and masks.
    seeds (a sequence of ints): an ensemble of S = st.members = len(seeds) simulations instead, every buffer but the frame
    counter with a leading member axis (state (S, capacity, .), waypoints (S, D, capacity, 2), records (S, T, capacity, .),
    spawned (S, 2), dropped (S), features (S, capacity, k, 6)); `seed` is then unused.  A single run has st.members None
    and is the one member of its launch: st.seeds holds the 64-bit patterns of the seed or seeds as a device int64 tensor,
    and st.rules the scene's piml_scenario_rules (GC's all-zero one for GC)."""
    dev = scenario.entries.device
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'scenario_state: the scenario must be on a GPU (piml_amd has no CPU path), got {dev}')
    cap, T, D = int(capacity), int(frames), int(scenario.num_waypoints)
    if cap < 1 or T < 1:
        raise ValueError(f'capacity and frames must be >= 1, got {cap}, {T}')
    st = types.SimpleNamespace(scenario=scenario, capacity=cap, T=T, seed=int(seed), members=None)
    lead = ()
    if seeds is not None:
        seeds = [int(x) for x in seeds]
        if not 1 <= len(seeds) <= MAX_MEMBERS:
            raise ValueError(f'seeds: 1 .. {MAX_MEMBERS} of them expected, got {len(seeds)}')
        st.members, st.seed_list, lead = len(seeds), seeds, (len(seeds),)
    bits = [(x & 0xFFFFFFFFFFFFFFFF) - ((x & 0x8000000000000000) << 1) for x in (seeds or [int(seed)])]   # int64 patterns
    st.seeds = torch.tensor(bits, device=dev, dtype=torch.long)
    f32 = dict(device=dev, dtype=torch.float32)
    nan = float('nan')
    st.p = torch.full((*lead, cap, 2), nan, **f32)
    st.v = torch.zeros(*lead, cap, 2, **f32)
    st.a = torch.zeros(*lead, cap, 2, **f32)
    st.dest = torch.full((*lead, cap, 2), nan, **f32)
    st.hist = torch.zeros(*lead, cap, hist_width, **f32)
    st.selff = torch.zeros(*lead, cap, hist_width + 5, **f32)
    st.desired_speed = torch.zeros(*lead, cap, **f32)
    st.mask = torch.zeros(*lead, cap, **f32)
    st.flag = torch.zeros(*lead, cap, device=dev, dtype=torch.int32)
    st.waypoints = torch.full((*lead, D, cap, 2), nan, **f32)
    st.exit_idx = torch.zeros(*lead, D, cap, device=dev, dtype=torch.int32)
    st.spawn_iters = torch.zeros(*lead, cap, device=dev, dtype=torch.int32)
    st.p_res = torch.full((*lead, T, cap, 2), nan, **f32)
    st.v_res = torch.zeros(*lead, T, cap, 2, **f32)
    st.a_res = torch.zeros(*lead, T, cap, 2, **f32)
    st.dest_res = torch.full((*lead, T, cap, 2), nan, **f32)
    st.mask_res = torch.zeros(*lead, T, cap, **f32)
    st.spawn_count = torch.zeros(*lead, T, device=dev, dtype=torch.int32)
    st.t = torch.zeros(1, device=dev, dtype=torch.long)
    st.spawned = torch.zeros(*lead, 2, device=dev, dtype=torch.long)
    st.dropped = torch.zeros(lead[0] if lead else 1, device=dev, dtype=torch.long)
    # feature buffers the relative-feature kernel writes (ops.relative_features_into)
    kp, ko = min(topk_ped, cap), min(topk_obs, scenario.obstacles.shape[0])
    st.pf = torch.empty(*lead, cap, kp, 6, **f32)
    st.of = torch.empty(*lead, cap, ko, 6, **f32)
    st.ped_idx = torch.empty(*lead, cap, kp, device=dev, dtype=torch.int32)
    st.obs_idx = torch.empty(*lead, cap, ko, device=dev, dtype=torch.int32)

    s = _lib.Scenario()
    for name, t in (('position', st.p), ('velocity', st.v), ('acceleration', st.a), ('destination', st.dest),
                    ('hist_velocity', st.hist), ('self_features', st.selff), ('desired_speed', st.desired_speed),
                    ('mask', st.mask), ('flag', st.flag), ('waypoints', st.waypoints), ('exit_idx', st.exit_idx),
                    ('spawn_iters', st.spawn_iters), ('position_out', st.p_res), ('velocity_out', st.v_res),
                    ('acceleration_out', st.a_res), ('destination_out', st.dest_res), ('mask_out', st.mask_res),
                    ('spawn_out', st.spawn_count), ('frame_counter', st.t), ('spawned', st.spawned), ('dropped', st.dropped),
                    ('entries', scenario.entries), ('route_polyline', scenario.route_polyline)):
        setattr(s, name, t.data_ptr())
    E, P = scenario.entries.shape[0], scenario.entries.shape[1]
    s.hist_width, s.F, s.D, s.E, s.P, s.R = hist_width, hist_width + 5, D, E, P, scenario.route_polyline.shape[0]
    s.capacity, s.T, s.n_initial = cap, T, int(scenario.n_initial)
    s.route_max_iters, s.spawn_cap, s.uniform_speed = int(scenario.route_max_iters), int(scenario.spawn_cap), int(bool(scenario.uniform_desired_speed))
    s.dt, s.spawn_offset, s.route_clearance = float(scenario.time_unit), float(scenario.spawn_offset), float(scenario.route_clearance)
    s.arrival_radius, s.speed_mean, s.speed_min = float(scenario.arrival_radius), float(scenario.speed_mean), float(scenario.speed_min)
    s.speed_std = float(scenario.speed_var ** 0.5)
    s.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    thr = scenario.poisson_thresholds()
    if len(thr) > 8:
        raise ValueError(f'spawn_cap {len(thr)} > 8')
    for j, x in enumerate(thr):
        s.poisson_thresholds[j] = x
    st.desc = s
    st.rules = scenario_rules(scenario) if scenario.spawn_law != 'gc' else _lib.ScenarioRules()
    return st


def scenario_state_reset(st):
    """Put the buffers of scenario_state back to what it allocated them as, in place (the addresses a captured graph
    holds stay valid): absent slots, empty records, frame counter and spawn counts 0.  Then scenario_step(st, init=True)
    starts the same simulation again."""
    nan = float('nan')
    for x in (st.p, st.dest, st.waypoints, st.p_res, st.dest_res):
        x.fill_(nan)
    for x in (st.v, st.a, st.hist, st.selff, st.desired_speed, st.mask, st.flag, st.exit_idx, st.spawn_iters, st.v_res,
              st.a_res, st.mask_res, st.spawn_count, st.t, st.spawned, st.dropped):
        x.zero_()


def scenario_rules(scenario):
    """The piml_scenario_rules descriptor of a scene (its spawn law, arrival rule, velocity and speed laws, second stream).
    The 'clip' law's track table is the scene's `entries`, which scenario_state puts into the piml_scenario descriptor."""
    r = _lib.ScenarioRules()
    if scenario.spawn_law not in _lib.SPAWN_LAWS or scenario.arrival_rule not in _lib.ARRIVAL_RULES:
        raise ValueError(f'unknown scene rule {scenario.spawn_law!r} / {scenario.arrival_rule!r}')
    r.spawn_law, r.arrival_rule = _lib.SPAWN_LAWS[scenario.spawn_law], _lib.ARRIVAL_RULES[scenario.arrival_rule]
    r.initial_velocity, r.speed_clamp = int(bool(scenario.initial_velocity)), int(bool(scenario.speed_clamp))
    r.length, r.width = float(scenario.length), float(scenario.width)
    r.side_ratio, r.direction_ratio = float(scenario.side_ratio), float(scenario.direction_ratio)
    thr = scenario.poisson_thresholds2()
    if len(thr) > 8:
        raise ValueError(f'spawn_cap2 {len(thr)} > 8')
    r.spawn_cap2 = len(thr)
    for j, x in enumerate(thr):
        r.poisson_thresholds2[j] = x
    if scenario.square_grid is not None:
        g = scenario.square_grid.detach().to('cpu', torch.float32).reshape(-1)
        if g.numel() > 32:
            raise ValueError(f'square grid of {g.numel()} > 32 cells per side')
        r.grid = g.numel()
        for j, x in enumerate(g.tolist()):
            r.square_grid[j] = x
    return r


def scenario_step(st, a_next=None, init=False):
    """One launch: init=True spawns the scenario's n_initial agents into frame st.t; otherwise frame st.t -> st.t + 1 with
    the network's accelerations a_next (capacity, 2), or (S, capacity, 2) for an ensemble state (every member in the same
    launch).  The caller advances st.t (ops.relative_features_into(tick=st.t))."""
    if not init:
        a_next = _gpu_f32('a_next', a_next)
        want = (st.capacity, 2) if st.members is None else (st.members, st.capacity, 2)
        if tuple(a_next.shape) != want or a_next.device != st.p.device:
            raise ValueError(f'a_next: {want} on {st.p.device} expected, got {tuple(a_next.shape)} on {a_next.device}')
    with torch.cuda.device(st.p.device):
        _lib.check(_lib.lib().piml_scenario_step_members(ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(),
                                                         _ptr(st.seeds), _ptr(a_next) if not init else None,
                                                         int(bool(init)), _stream()), 'piml_scenario_step_members')


def mlapm_law(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0, radius=0.3):
    """The piml_mlapm_law of MLAPM(version, tau, A, B, C, D, theta) (defaults: src/main_mlapm.py:16's constants).
    radius is MLAPM.step's (the UCY collision radius, mlapm.py:42-46), not the scene's arrival radius.  ValueError for an
    unknown version, tau not finite and > 0, a non-finite constant or radius not finite and > 0."""
    from .ops import MLAPM_VARIANTS
    if version not in MLAPM_VARIANTS:
        raise ValueError(f'MLAPM version {version!r} unknown (one of {sorted(MLAPM_VARIANTS)})')
    vals = dict(tau=tau, A=A, B=B, C=C, D=D, theta=theta, radius=radius)
    for k, x in vals.items():
        if not math.isfinite(float(x)):
            raise ValueError(f'MLAPM {k} = {x} is not finite')
    if not float(tau) > 0 or not float(radius) > 0:
        raise ValueError(f'MLAPM tau and radius must be > 0, got tau={tau}, radius={radius}')
    law = _lib.MlapmLaw()
    law.variant = MLAPM_VARIANTS[version]
    law.tau, law.A, law.B, law.C, law.D = float(tau), float(A), float(B), float(C), float(D)
    law.theta_deg, law.radius = float(theta), float(radius)
    return law


def mlapm_law_table_host(laws):
    """The law table of a list of mlapm_law(...) as a CPU uint8 tensor (piml_mlapm_law_table_fill: host to host, no GPU call):
    row m holds law m's derived constants, formed by the code that forms the single-law launch's.  ValueError on an empty
    list or a law the library rejects (the bytes are then not produced)."""
    laws = list(laws)
    if not laws:
        raise ValueError('mlapm_law_table: at least one law expected')
    for law in laws:
        if not isinstance(law, _lib.MlapmLaw):
            raise TypeError(f'laws: ops_scenario.mlapm_law(...) values expected, got {type(law).__name__}')
    L = _lib.lib()
    arr = (_lib.MlapmLaw * len(laws))(*laws)
    host = torch.zeros(int(L.piml_mlapm_law_table_bytes(len(laws))), dtype=torch.uint8)
    if L.piml_mlapm_law_table_fill(arr, len(laws), host.data_ptr()) != 0:
        raise ValueError('mlapm_law_table: a law is out of range (variant 0..2, finite constants, tau > 0, radius > 0)')
    return host


def mlapm_law_table(laws, device='cuda', out=None):
    """The law table of piml_scenario_step_mlapm_laws for a list of mlapm_law(...): a (len(laws), row bytes) device uint8
    tensor, one host fill and one copy.  out: a table of the same shape to overwrite in place instead (a captured run
    reads the buffer at every replay, so this changes the laws of the frames replayed afterwards)."""
    host = mlapm_law_table_host(laws)
    host = host.view(len(laws), -1)
    if out is not None:
        if out.dtype != torch.uint8 or tuple(out.shape) != tuple(host.shape) or not out.is_contiguous():
            raise ValueError(f'out: a contiguous uint8 table {tuple(host.shape)} expected, got {out.dtype} {tuple(out.shape)}')
        out.copy_(host)
        return out
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'mlapm_law_table: a GPU device expected (piml_amd has no CPU path), got {dev}')
    return host.to(dev)


def scenario_step_mlapm(st, law, frame_offset=0, advance=True):
    """One launch: frame t -> t + 1 of st (single or ensemble state) under the MLAPM law `law` (mlapm_law(...)), t =
    st.t + frame_offset: the force of MLAPM.step from the agents present in frame t's records, v' = v + F dt, p' = p + v' dt
    (src/main_mlapm.py:18-36), a' = F, then the scene's arrivals, exits and spawns as scenario_step.  advance: add 1 to
    st.t afterwards (the kernel reads the counter, never writes it; a captured run of K frames passes offsets 0 .. K-1 and
    advances once by K).  Frame 0's spawn is scenario_step(st, init=True), which does not depend on the law.
    law may instead be a table of mlapm_law_table(...) with one row per member of st (member m steps under row m,
    piml_scenario_step_mlapm_laws); ValueError when it does not hold exactly st.seeds.numel() rows or is on another device."""
    table = isinstance(law, torch.Tensor)
    if table:
        row = int(_lib.lib().piml_mlapm_law_table_bytes(1))
        if law.dtype != torch.uint8 or law.dim() != 2 or law.shape[1] != row or not law.is_contiguous():
            raise ValueError(f'law table: a contiguous uint8 (members, {row}) tensor of mlapm_law_table expected, got '
                             f'{law.dtype} {tuple(law.shape)}')
        if law.shape[0] != st.seeds.numel():
            raise ValueError(f'law table: {law.shape[0]} rows for {st.seeds.numel()} members')
        if law.device != st.p.device:
            raise ValueError(f'law table on {law.device}, the state on {st.p.device}')
    elif not isinstance(law, _lib.MlapmLaw):
        raise TypeError(f'law: an ops_scenario.mlapm_law(...) or a mlapm_law_table(...) expected, got {type(law).__name__}')
    if int(frame_offset) < 0:
        raise ValueError(f'frame_offset must be >= 0, got {frame_offset}')
    with torch.cuda.device(st.p.device):
        if table:
            _lib.check(_lib.lib().piml_scenario_step_mlapm_laws(ctypes.byref(st.desc), ctypes.byref(st.rules),
                                                                st.seeds.numel(), _ptr(st.seeds), _ptr(law),
                                                                int(frame_offset), _stream()), 'piml_scenario_step_mlapm_laws')
        else:
            _lib.check(_lib.lib().piml_scenario_step_mlapm(ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(),
                                                           _ptr(st.seeds), ctypes.byref(law), int(frame_offset), _stream()),
                       'piml_scenario_step_mlapm')
        if advance:
            st.t.add_(1)
