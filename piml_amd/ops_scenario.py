"""Open-world scenario operators over the C ABI (include/piml_hip.h: piml_scenario_step, piml_scenario_step_rules,
piml_scenario_step_members, piml_scenario_step_nav, piml_scenario_step_mlapm, piml_scenario_step_mlapm_laws, piml_scenario_step_mlapm_walls,
piml_wall_force, piml_scenario_step_mlapm_groups, piml_group_force, piml_scenario_step_mlapm_noise, piml_noise_force,
piml_nav_relax, piml_nav_direction, piml_scenario_step_mlapm_nav, piml_nav_density, piml_nav_cost, piml_nav_relax_cost,
piml_nav_descent, piml_nav_flow, piml_nav_cost_flow, piml_nav_relax_cost_gates, piml_nav_relax_active,
piml_scenario_step_mlapm_navdyn, piml_nav_choose_exit, piml_scenario_route).

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
    and st.rules the scene's piml_scenario_rules (GC's all-zero one for GC).  A grouped clip scene ('clip_groups') also
    gets st.group_first / st.group_size ((S,) capacity int32, zero: per slot the first slot and the size of its unit) and
    st.groups, the piml_scene_groups over them and the scene's row_unit / unit_rows.  st.noise_state is None until a frame
    with the fluctuation term needs it (scenario_noise_state: (S,) capacity, 2 float32 zeros, eta of every slot), st.steer
    None until a frame routed by a floor field writes it (scenario_step(nav=): (S,) capacity, 2 float32, NaN), st.exit_switches
    None until a run with an exit choice counts its switches (scenario_exit_switches: (S,) capacity int32 zeros)."""
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
    st.groups = None
    st.noise_state = None
    st.steer = None
    st.exit_switches = None
    if scenario.spawn_law == 'clip_groups':
        ru, ur = scenario.row_unit, scenario.unit_rows
        if ru is None or ur is None or ru.dtype != torch.int32 or ur.dtype != torch.int32 or ru.device != dev or \
                ur.device != dev or tuple(ru.shape) != (E, 2) or ur.dim() != 1 or not (ru.is_contiguous() and ur.is_contiguous()):
            raise ValueError(f"a 'clip_groups' scene needs row_unit ({E}, 2) and unit_rows (Ua,) int32 on {dev} (Scenario.to)")
        st.group_first = torch.zeros(*lead, cap, device=dev, dtype=torch.int32)
        st.group_size = torch.zeros(*lead, cap, device=dev, dtype=torch.int32)
        st.unit_rows = ur if ur.numel() else torch.zeros(1, device=dev, dtype=torch.int32)   # (the entry takes no NULL)
        g = _lib.SceneGroups()
        g.row_unit, g.unit_rows, g.n_units = ru.data_ptr(), st.unit_rows.data_ptr(), int(ur.numel())
        g.group_first, g.group_size = st.group_first.data_ptr(), st.group_size.data_ptr()
        st.groups = g
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
    if getattr(st, 'groups', None) is not None:
        st.group_first.zero_()
        st.group_size.zero_()
    if getattr(st, 'noise_state', None) is not None:
        st.noise_state.zero_()
    if getattr(st, 'steer', None) is not None:
        st.steer.fill_(nan)
    if getattr(st, 'exit_switches', None) is not None:
        st.exit_switches.zero_()


def scenario_noise_state(st):
    """The fluctuation term's state of st, eta per slot ((S,) capacity, 2 float32), allocated as zeros when first needed and
    kept (scenario_state_reset zeroes it in place: eta = 0 at birth)."""
    if getattr(st, 'noise_state', None) is None:
        st.noise_state = torch.zeros_like(st.v)
    return st.noise_state


def scenario_rules(scenario):
    """The piml_scenario_rules descriptor of a scene (its spawn law, arrival rule, velocity and speed laws, second stream).
    The 'clip' law's track table is the scene's `entries`, which scenario_state puts into the piml_scenario descriptor."""
    r = _lib.ScenarioRules()
    laws = dict(_lib.SPAWN_LAWS, clip_groups=_lib.SPAWN_CLIP_GROUPS)
    if scenario.spawn_law not in laws or scenario.arrival_rule not in _lib.ARRIVAL_RULES:
        raise ValueError(f'unknown scene rule {scenario.spawn_law!r} / {scenario.arrival_rule!r}')
    r.spawn_law, r.arrival_rule = laws[scenario.spawn_law], _lib.ARRIVAL_RULES[scenario.arrival_rule]
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


def scenario_step(st, a_next=None, init=False, nav=None):
    """One launch: init=True spawns the scenario's n_initial agents into frame st.t; otherwise frame st.t -> st.t + 1 with
    the network's accelerations a_next (capacity, 2), or (S, capacity, 2) for an ensemble state (every member in the same
    launch).  The caller advances st.t (ops.relative_features_into(tick=st.t)).  ValueError for a grouped clip scene
    ('clip_groups'): its frames, the init launch included, are scenario_step_mlapm's.
    nav = a nav_field(...) of the scene: the same frame through piml_scenario_step_nav, which also writes st.steer ((S,)
    capacity, 2): per present slot the point one metre down the floor field from its new position -- position +
    nav_direction(position, exit_idx[flag], destination), the destination itself in the lookup's branch 0 --, NaN for absent
    and retired slots.  Handed to ops.relative_features_into in the place of st.dest it steers a PINNSF, which reads the
    destination as a direction only; position, records and arrivals are the frame's without the field, bit for bit.  A field
    with the any-angle table is looked up through it.  st.steer is allocated (NaN) at the first such call, the init launch,
    and scenario_state_reset refills it.  TypeError unless nav is a NavField; ValueError (check_nav_scene) for a scene rule
    other than GC's, route_max_iters != 0, or a field of another number of gates."""
    if nav is not None:
        _check_nav(st, nav)
        if isinstance(nav, NavFieldDynamic):
            raise NotImplementedError('scenario_step: a field per member (NavFieldDynamic) is not built for the network-driven '
                                      'frame; scenario_step_mlapm has it')
    if getattr(st, 'groups', None) is not None:
        raise ValueError("scenario_step: a 'clip_groups' scene runs under the MLAPM frame only (scenario_step_mlapm)")
    if not init:
        a_next = _gpu_f32('a_next', a_next)
        want = (st.capacity, 2) if st.members is None else (st.members, st.capacity, 2)
        if tuple(a_next.shape) != want or a_next.device != st.p.device:
            raise ValueError(f'a_next: {want} on {st.p.device} expected, got {tuple(a_next.shape)} on {a_next.device}')
    if nav is not None:
        if getattr(st, 'steer', None) is None:
            st.steer = torch.full_like(st.p, float('nan'))
        with torch.cuda.device(st.p.device):
            _lib.check(_lib.lib().piml_scenario_step_nav(
                ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds),
                _ptr(a_next) if not init else None, int(bool(init)), ctypes.byref(nav.desc),
                None if nav.sight_desc is None else ctypes.byref(nav.sight_desc), _ptr(st.steer), _stream()),
                'piml_scenario_step_nav')
        return
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


WALL_CELL_MARGIN = 1.0 + 2.0 ** -5     # cell >= cutoff (1 + 2^-5): the 3 x 3 neighbourhood's exactness margin (walls.hpp)
WALL_MAX_CELLS = 1024                  # per axis


def wall_law(Aw, Bw):
    """The piml_wall_law of W = Aw exp(Bw d) n (include/piml_hip.h).  ValueError unless both are finite, Aw >= 0, Bw <= 0."""
    Aw, Bw = float(Aw), float(Bw)
    if not (math.isfinite(Aw) and math.isfinite(Bw)) or Aw < 0 or Bw > 0:
        raise ValueError(f'wall law: finite Aw >= 0 and Bw <= 0 expected, got Aw={Aw}, Bw={Bw}')
    law = _lib.WallLaw()
    law.A, law.B = Aw, Bw
    return law


def wall_grid_host(obstacles, cutoff=2.0):
    """The static cell grid of a scene's obstacle points, on the host in numpy (no GPU call): a namespace of
    points (n, 2) float32 -- the valid points (both coordinates finite) sorted stably by cell index cy gx + cx --, order (n)
    the sorted points' indices into `obstacles`, cell_start (gx gy + 1) int32 CSR offsets, n_points, gx, gy and the float32
    scalars x0, y0 (the points' minimum), cell, cutoff.  A point's cell is floor((q - origin) / cell) in float32;
    cell = cutoff (1 + 2^-5), coarsened (with a warning) when that would need more than 1024 cells per axis.
    ValueError unless cutoff is finite and > 0."""
    import numpy as np
    f32 = np.float32
    if not math.isfinite(float(cutoff)) or not float(cutoff) > 0:
        raise ValueError(f'wall_grid: a finite cutoff > 0 expected, got {cutoff}')
    if isinstance(obstacles, torch.Tensor):
        obstacles = obstacles.detach().cpu().numpy()
    obs = np.ascontiguousarray(np.asarray(obstacles, dtype=f32).reshape(-1, 2))
    keep = np.flatnonzero(np.isfinite(obs).all(1))
    pts = obs[keep]
    cutoff = f32(cutoff)
    cell = f32(cutoff * f32(WALL_CELL_MARGIN))
    g = types.SimpleNamespace(cutoff=float(cutoff), n_points=int(pts.shape[0]))
    if pts.shape[0] == 0:
        g.points, g.order = pts, keep
        g.cell_start = np.zeros(2, np.int32)
        g.gx = g.gy = 1
        g.x0 = g.y0 = 0.0
        g.cell = float(cell)
        return g
    origin = pts.min(0)
    span = float((pts.max(0).astype(np.float64) - origin).max())
    if span / float(cell) >= WALL_MAX_CELLS - 1:
        import warnings
        coarse = f32(span / (WALL_MAX_CELLS - 2))
        warnings.warn(f'wall_grid: the obstacles span {span:g} m, more than {WALL_MAX_CELLS} cells of {float(cell):g} m per '
                      f'axis: cells coarsened to {float(coarse):g} m')
        cell = max(cell, coarse)
    c = np.floor((pts - origin) / cell).astype(np.int64)
    gx, gy = int(c[:, 0].max()) + 1, int(c[:, 1].max()) + 1
    if gx > WALL_MAX_CELLS or gy > WALL_MAX_CELLS:
        raise ValueError(f'wall_grid: {gx} x {gy} cells (more than {WALL_MAX_CELLS} per axis)')
    key = c[:, 1] * gx + c[:, 0]
    order = np.argsort(key, kind='stable')
    g.points = np.ascontiguousarray(pts[order])
    g.order = keep[order]
    g.cell_start = np.concatenate(([0], np.cumsum(np.bincount(key, minlength=gx * gy)))).astype(np.int32)
    g.gx, g.gy, g.x0, g.y0, g.cell = gx, gy, float(origin[0]), float(origin[1]), float(cell)
    return g


def wall_grid(obstacles, cutoff=2.0, device='cuda'):
    """wall_grid_host's grid with its points and cell_start on `device` and the piml_wall_grid descriptor that points at
    them: a namespace of points, cell_start (device tensors), desc, cutoff, cell, gx, gy, x0, y0, n_points and host (the
    wall_grid_host namespace: the numpy copies and `order`).  Built once per scene; the obstacles are static."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'wall_grid: a GPU device expected (piml_amd has no CPU path), got {dev}')
    h = wall_grid_host(obstacles, cutoff)
    g = types.SimpleNamespace(host=h, cutoff=h.cutoff, cell=h.cell, gx=h.gx, gy=h.gy, x0=h.x0, y0=h.y0, n_points=h.n_points)
    g.points = torch.from_numpy(h.points).to(dev)
    g.cell_start = torch.from_numpy(h.cell_start).to(dev)
    g.desc = wall_grid_desc(h, g.points.data_ptr() if h.n_points else None, g.cell_start.data_ptr())
    return g


def wall_grid_desc(h, points_ptr, cell_start_ptr):
    """The piml_wall_grid of a wall_grid_host namespace over the given buffers."""
    d = _lib.WallGrid()
    d.points, d.cell_start = points_ptr, cell_start_ptr
    d.n_points, d.gx, d.gy = h.n_points, h.gx, h.gy
    d.x0, d.y0, d.cell, d.cutoff = h.x0, h.y0, h.cell, h.cutoff
    return d


def wall_force(position, grid, Aw, Bw, return_selection=False):
    """The wall term W = Aw exp(Bw d) (p - q*) / d of every row of position (..., 2) against the nearest valid obstacle point
    q* within grid.cutoff (wall_grid(...); piml_wall_force, one wave per row): force (..., 2), zero where no point is felt
    (none within the cutoff, a NaN position, d == 0).  return_selection: also dist2 (...) float32 (the exact squared
    distance, +inf for none) and index (...) int32 into grid.points (grid.host.order maps it to the obstacle list; -1 for
    none)."""
    law = wall_law(Aw, Bw)
    p = _gpu_f32('position', position)
    if p.dim() < 1 or p.shape[-1] != 2:
        raise ValueError(f'position: (..., 2) expected, got {tuple(p.shape)}')
    if grid.cell_start.device != p.device:
        raise ValueError(f'position on {p.device}, the wall grid on {grid.cell_start.device}')
    lead = p.shape[:-1]
    rows = p.numel() // 2
    force = torch.zeros_like(p)
    dist2 = torch.full(lead, float('inf'), device=p.device, dtype=torch.float32) if return_selection else None
    index = torch.full(lead, -1, device=p.device, dtype=torch.int32) if return_selection else None
    if rows and grid.n_points:                   # (an empty problem keeps the fills above: the entry launches nothing)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().piml_wall_force(_ptr(p), rows, ctypes.byref(grid.desc), law.A, law.B, _ptr(force),
                                                  _ptr(dist2), _ptr(index), _stream()), 'piml_wall_force')
    return (force, dist2, index) if return_selection else force


def wall_law_table(rows, device='cuda', out=None):
    """The wall table of piml_scenario_step_mlapm_walls: rows, a list of (Aw, Bw) pairs or wall_law(...) values, one per
    member, as a (len(rows), 2) float32 device tensor (every row checked as wall_law does).  out: a table of the same
    shape to overwrite in place instead (a captured run reads the buffer at every replay)."""
    laws = [r if isinstance(r, _lib.WallLaw) else wall_law(*r) for r in rows]
    if not laws:
        raise ValueError('wall_law_table: at least one row expected')
    host = torch.tensor([[w.A, w.B] for w in laws], dtype=torch.float32)
    if out is not None:
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(host.shape) or not out.is_contiguous():
            raise ValueError(f'out: a contiguous float32 table {tuple(host.shape)} expected, got {out.dtype} {tuple(out.shape)}')
        out.copy_(host)
        return out
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'wall_law_table: a GPU device expected (piml_amd has no CPU path), got {dev}')
    return host.to(dev)


def group_law(Ag, dist=0.5):
    """The piml_group_law of the group term (include/piml_hip.h): a pull of Ag m/s^2 towards the centroid of the agent's
    group once it is further from it than dist (n - 1) m.  ValueError unless both are finite and >= 0."""
    Ag, dist = float(Ag), float(dist)
    if not (math.isfinite(Ag) and math.isfinite(dist)) or Ag < 0 or dist < 0:
        raise ValueError(f'group law: finite Ag >= 0 and dist >= 0 expected, got Ag={Ag}, dist={dist}')
    law = _lib.GroupLaw()
    law.A, law.dist = Ag, dist
    return law


def group_law_table(rows, device='cuda', out=None):
    """The group table of piml_scenario_step_mlapm_groups: rows, a list of (Ag, dist) pairs or group_law(...) values, one per
    member, as a (len(rows), 2) float32 device tensor (every row checked as group_law does).  out: a table of the same
    shape to overwrite in place instead (a captured run reads the buffer at every replay)."""
    laws = [r if isinstance(r, _lib.GroupLaw) else group_law(*r) for r in rows]
    if not laws:
        raise ValueError('group_law_table: at least one row expected')
    host = torch.tensor([[g.A, g.dist] for g in laws], dtype=torch.float32)
    if out is not None:
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(host.shape) or not out.is_contiguous():
            raise ValueError(f'out: a contiguous float32 table {tuple(host.shape)} expected, got {out.dtype} {tuple(out.shape)}')
        out.copy_(host)
        return out
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'group_law_table: a GPU device expected (piml_amd has no CPU path), got {dev}')
    return host.to(dev)


def group_force(position, group_first, group_size, Ag, dist=0.5):
    """The group term G of every slot of position (..., N, 2) (piml_group_force, one thread per row; include/piml_hip.h):
    slot i's mates are the slots [group_first[i], group_first[i] + group_size[i]) of its own (N, 2) block, clamped to
    [0, N), present when their position is not NaN; G = Ag e / |e| towards the present mates' centroid when |e| > dist
    (n - 1), else 0 (also for a NaN position and for fewer than two present mates).  group_first, group_size: int32 (N) or
    (..., N) (broadcast over the leading axes), as a result's or ensemble's .group_first / .group_size.  Bitwise what the
    frame adds for a frame whose recorded positions are `position`."""
    law = group_law(Ag, dist)
    p = _gpu_f32('position', position)
    if p.dim() < 2 or p.shape[-1] != 2:
        raise ValueError(f'position: (..., N, 2) expected, got {tuple(p.shape)}')
    N = p.shape[-2]
    gf = torch.as_tensor(group_first, device=p.device).to(torch.int32)
    gs = torch.as_tensor(group_size, device=p.device).to(torch.int32)
    if gf.shape[-1:] != (N,) or gs.shape[-1:] != (N,):
        raise ValueError(f'group_first / group_size: (..., {N}) expected, got {tuple(gf.shape)}, {tuple(gs.shape)}')
    if p.dim() > 2:                                  # blocks of N rows: clamp to the block here, then shift to flat rows
        gf, gs = gf.expand(p.shape[:-1]), gs.expand(p.shape[:-1])
        lo, hi = gf.long().clamp(min=0), (gf.long() + gs.long()).clamp(max=N)
        block = torch.arange(p.numel() // (2 * N), device=p.device).reshape(*p.shape[:-2], 1) * N
        gf, gs = (lo + block).to(torch.int32), (hi - lo).clamp(min=0).to(torch.int32)
        if p.numel() // 2 > 0x7fffffff:
            raise ValueError(f'position: {p.numel() // 2} rows, more than 2^31 - 1')
    gf, gs = gf.contiguous(), gs.contiguous()
    force = torch.zeros_like(p)
    rows = p.numel() // 2
    if rows:
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().piml_group_force(_ptr(p), _ptr(gf), _ptr(gs), rows, law.A, law.dist, _ptr(force),
                                                   _stream()), 'piml_group_force')
    return force


def noise_law(An, noise_tau, dt):
    """The piml_noise_law (rho, amp) of the fluctuation term eta' = rho eta + amp z (include/piml_hip.h): rho = exp(-dt /
    noise_tau), 0 for noise_tau == 0 (white noise, eta = An z), amp = An sqrt(1 - rho^2), both formed in float64 and rounded
    to float32 once.  An (m/s^2) is the stationary standard deviation of each component of eta; with noise_tau == 0 the
    per-frame acceleration has standard deviation An whatever dt is (the velocity kick An dt is NOT a Wiener increment).
    ValueError unless all three are finite, An >= 0, noise_tau >= 0 and dt > 0, or when noise_tau is so long that rho rounds
    to 1 in float32."""
    An, noise_tau, dt = float(An), float(noise_tau), float(dt)
    if not (math.isfinite(An) and math.isfinite(noise_tau) and math.isfinite(dt)) or An < 0 or noise_tau < 0 or not dt > 0:
        raise ValueError(f'noise law: finite An >= 0, noise_tau >= 0 and dt > 0 expected, got An={An}, noise_tau={noise_tau}, '
                         f'dt={dt}')
    rho = math.exp(-dt / noise_tau) if noise_tau > 0 else 0.0
    law = _lib.NoiseLaw()
    law.rho, law.amp = rho, An * math.sqrt(1.0 - rho * rho)
    if not law.rho < 1.0:
        raise ValueError(f'noise law: noise_tau={noise_tau} is too long for dt={dt} (rho rounds to 1 in float32)')
    return law


def noise_law_table(rows, dt, device='cuda', out=None):
    """The noise table of piml_scenario_step_mlapm_noise: rows, a list of (An, noise_tau) pairs or noise_law(...) values, one
    per member, as a (len(rows), 2) float32 device tensor of (rho, amp) (every pair formed as noise_law does with `dt`).
    out: a table of the same shape to overwrite in place instead (a captured run reads the buffer at every replay)."""
    laws = [r if isinstance(r, _lib.NoiseLaw) else noise_law(r[0], r[1], dt) for r in rows]
    if not laws:
        raise ValueError('noise_law_table: at least one row expected')
    host = torch.tensor([[w.rho, w.amp] for w in laws], dtype=torch.float32)
    if out is not None:
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(host.shape) or not out.is_contiguous():
            raise ValueError(f'out: a contiguous float32 table {tuple(host.shape)} expected, got {out.dtype} {tuple(out.shape)}')
        out.copy_(host)
        return out
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'noise_law_table: a GPU device expected (piml_amd has no CPU path), got {dev}')
    return host.to(dev)


def noise_force(eta, seeds, frame, An, noise_tau, dt, present=None, return_draws=False):
    """One step of the fluctuation term for every row of eta ((members,) N, 2) (piml_noise_force, one thread per row): row
    (m, i) draws two standard normals z for (seeds[m], frame, slot i) and gets rho eta + amp z with noise_law(An, noise_tau,
    dt)'s constants.  seeds: one int, or `members` of them (64-bit patterns, as scenario_state takes them).  present
    ((members,) N, anything whose != 0 marks a live slot; None: all): a row that is not present keeps its eta and draws
    nothing (z = 0).  Returns the new eta, and z with return_draws.  Bitwise what the frame leaves in its state and adds to
    the force for the step from frame `frame`."""
    law = noise_law(An, noise_tau, dt)
    e = _gpu_f32('eta', eta)
    if e.dim() not in (2, 3) or e.shape[-1] != 2:
        raise ValueError(f'eta: ((members,) N, 2) expected, got {tuple(e.shape)}')
    members, N = (1 if e.dim() == 2 else e.shape[0]), e.shape[-2]
    seeds = [int(seeds)] if isinstance(seeds, int) else [int(x) for x in (seeds.tolist() if isinstance(seeds, torch.Tensor) else seeds)]
    if len(seeds) != members:
        raise ValueError(f'seeds: {members} expected, got {len(seeds)}')
    if int(frame) < 0:
        raise ValueError(f'frame must be >= 0, got {frame}')
    bits = [(x & 0xFFFFFFFFFFFFFFFF) - ((x & 0x8000000000000000) << 1) for x in seeds]
    sd = torch.tensor(bits, device=e.device, dtype=torch.long)
    pr = None
    if present is not None:
        pr = (torch.as_tensor(present, device=e.device) != 0).to(torch.uint8).contiguous()
        if tuple(pr.shape) != tuple(e.shape[:-1]):
            raise ValueError(f'present: {tuple(e.shape[:-1])} expected, got {tuple(pr.shape)}')
    out = torch.empty_like(e)
    z = torch.empty_like(e) if return_draws else None
    if e.numel():
        with torch.cuda.device(e.device):
            _lib.check(_lib.lib().piml_noise_force(_ptr(out), _ptr(z), _ptr(e), _ptr(pr), _ptr(sd), members, N, int(frame),
                                                   law.rho, law.amp, _stream()), 'piml_noise_force')
    return (out, z) if return_draws else out


def _group_arg_is_table(st, groups):
    """scenario_step_mlapm's check of `groups`; True for a table"""
    group_table = isinstance(groups, torch.Tensor)
    if group_table:
        if groups.dtype != torch.float32 or tuple(groups.shape) != (st.seeds.numel(), 2) or not groups.is_contiguous():
            raise ValueError(f'group table: a contiguous float32 ({st.seeds.numel()}, 2) tensor of group_law_table '
                             f'expected, got {groups.dtype} {tuple(groups.shape)}')
        if groups.device != st.p.device:
            raise ValueError(f'group table on {groups.device}, the state on {st.p.device}')
    elif groups is not None and not isinstance(groups, _lib.GroupLaw):
        raise TypeError(f'groups: a group_law or a group_law_table expected, got {type(groups).__name__}')
    return group_table


NAV_MAX_CELLS = 1024                   # per axis (nav.hpp)
NAV_MAX_GATES = 64
NAV_STEPS = 8                          # Jacobi steps of one piml_nav_relax launch
NAV_BATCH = 16                         # launches queued between two looks at `changed`
NAV_SIGHT_BATCH = 32                   # the same for piml_nav_sight_relax, whose launch is one step


def nav_grid_host(scenario, cell=0.25, bounds=None):
    """The floor field's grid over a scene of gates, on the host in numpy (no GPU call): a namespace of gx, gy and the
    float32 scalars x0, y0, cell, of centres (gy, gx, 2) float32 -- x0 + (i + 0.5) cell, the points `blocked` is decided at --
    and goal (G, gy, gx) uint8, the cells that hold gate g's sample points (a point's cell is floor((q - origin) / cell) in
    float32, the wall grid's formula).  bounds = (xmin, ymin, xmax, ymax); default: the box of the obstacles and gate points
    padded by spawn_offset + cell.  A box of more than 1024 cells per axis coarsens `cell`, with a warning.  ValueError for
    more than 64 gates, a cell not finite and > 0, an empty box, or a gate without a point inside the grid."""
    import numpy as np
    f32 = np.float32
    cell = float(cell)
    if not math.isfinite(cell) or not cell > 0:
        raise ValueError(f'nav_field: a finite cell > 0 expected, got {cell}')
    ent = scenario.entries.detach().cpu().numpy().astype(f32)
    if ent.ndim != 3 or ent.shape[0] < 1 or ent.shape[0] > NAV_MAX_GATES:
        raise ValueError(f'nav_field: 1 .. {NAV_MAX_GATES} gates (E, P, 2) expected, got entries {tuple(ent.shape)}')
    if bounds is None:
        obs = scenario.obstacles.detach().cpu().numpy().astype(f32).reshape(-1, 2)
        pts = np.concatenate([obs[np.isfinite(obs).all(1)], ent.reshape(-1, 2)])
        pad = float(scenario.spawn_offset) + cell
        lo, hi = pts.min(0).astype(np.float64) - pad, pts.max(0).astype(np.float64) + pad
    else:
        lo, hi = np.array(bounds[:2], np.float64), np.array(bounds[2:], np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f'nav_field: a finite, non-empty box expected, got {lo.tolist()} .. {hi.tolist()}')
    span = float((hi - lo).max())
    if span / cell > NAV_MAX_CELLS:
        import warnings
        coarse = span / (NAV_MAX_CELLS - 1)
        warnings.warn(f'nav_field: the box spans {span:g} m, more than {NAV_MAX_CELLS} cells of {cell:g} m per axis: cells '
                      f'coarsened to {coarse:g} m')
        cell = coarse
    g = types.SimpleNamespace(cell=float(f32(cell)), x0=float(f32(lo[0])), y0=float(f32(lo[1])))
    g.gx = min(NAV_MAX_CELLS, max(1, int(math.ceil((hi[0] - lo[0]) / g.cell))))
    g.gy = min(NAV_MAX_CELLS, max(1, int(math.ceil((hi[1] - lo[1]) / g.cell))))
    c, x0, y0 = f32(g.cell), f32(g.x0), f32(g.y0)
    cx = x0 + (np.arange(g.gx, dtype=f32) + f32(0.5)) * c
    cy = y0 + (np.arange(g.gy, dtype=f32) + f32(0.5)) * c
    g.centres = np.ascontiguousarray(np.stack(np.broadcast_arrays(cx[None, :], cy[:, None]), -1).astype(f32))
    g.goal = np.zeros((ent.shape[0], g.gy, g.gx), np.uint8)
    for e in range(ent.shape[0]):
        q = ent[e][np.isfinite(ent[e]).all(1)]
        ix, iy = np.floor((q[:, 0] - x0) / c), np.floor((q[:, 1] - y0) / c)
        keep = (ix >= 0) & (ix < g.gx) & (iy >= 0) & (iy < g.gy)
        if not keep.any():
            raise ValueError(f'nav_field: gate {e} has no point inside the grid')
        g.goal[e, iy[keep].astype(np.int64), ix[keep].astype(np.int64)] = 1
    return g


class NavField:
    """The static floor field of a scene of gates (nav_field): u (G, gy, gx) float32 -- gate g's geodesic distance over the
    free cells in CELL units, +inf on blocked and unreachable cells --, blocked (gy, gx) and goal (G, gy, gx) uint8, all on
    the device; desc the piml_nav_grid over u; G, gx, gy, x0, y0, cell, near, clearance; iterations, the Jacobi steps
    queued until a batch changed nothing.
    With the any-angle table (nav_field(..., sight=True)) also w (G, gy, gx) float32 and parent (G, gy, gx) int32 of
    nav_sight_relax, sight_desc the piml_nav_sight over parent, and sight_iterations, its steps; all None / 0 otherwise."""

    def __init__(self, u, blocked, goal, x0, y0, cell, near, clearance=None, iterations=0, *, w=None, parent=None,
                 sight_iterations=0):
        if not math.isfinite(float(near)) or float(near) < 0:
            raise ValueError(f'nav field: a finite near >= 0 (cells) expected, got {near}')
        self.u, self.blocked, self.goal = u, blocked, goal
        self.G, self.gy, self.gx = (int(n) for n in u.shape)
        self.x0, self.y0, self.cell, self.near = float(x0), float(y0), float(cell), float(near)
        self.clearance, self.iterations = clearance, int(iterations)
        d = _lib.NavGrid()
        d.u, d.G, d.gx, d.gy = u.data_ptr(), self.G, self.gx, self.gy
        d.x0, d.y0, d.cell, d.near = self.x0, self.y0, self.cell, self.near
        self.desc = d
        self.w, self.parent, self.sight_desc, self.sight_iterations = w, parent, None, int(sight_iterations)
        if parent is not None:
            if parent.dtype != torch.int32 or tuple(parent.shape) != tuple(u.shape) or parent.device != u.device \
                    or not parent.is_contiguous():
                raise ValueError(f'nav field: parent, a contiguous int32 {tuple(u.shape)} tensor on {u.device} expected, got '
                                 f'{parent.dtype} {tuple(parent.shape)} on {parent.device}')
            sd = _lib.NavSight()
            sd.parent, sd.G, sd.gx, sd.gy = parent.data_ptr(), self.G, self.gx, self.gy
            self.sight_desc = sd

    def to_numpy(self):
        """a namespace of the numpy copies u, blocked, goal and the scalars; with the any-angle table also w and parent"""
        out = types.SimpleNamespace(u=self.u.cpu().numpy(), blocked=self.blocked.cpu().numpy(), goal=self.goal.cpu().numpy(),
                                    G=self.G, gx=self.gx, gy=self.gy, x0=self.x0, y0=self.y0, cell=self.cell, near=self.near)
        if self.parent is not None:
            out.parent = self.parent.cpu().numpy()
            out.w = None if self.w is None else self.w.cpu().numpy()
        return out

    def reachable(self, g):
        """(gy, gx) bool: the cells gate g can be reached from (u[g] finite)"""
        return torch.isfinite(self.u[int(g)])


def nav_relax(blocked, goal, u=None, launches=None):
    """The eikonal solve of piml_nav_relax on device tensors: blocked (gy, gx) uint8, goal (G, gy, gx) uint8 -> (u (G, gy, gx)
    float32 in cell units, the number of Jacobi steps queued).  u: a start to step from (default 0 on goal cells, +inf
    elsewhere); it is not written.  launches = None: batches of 16 launches of 8 steps until a batch changed nothing (a fixed
    point: u only decreases); RuntimeError if gx gy steps were not enough.  launches = n: exactly n launches, wherever that
    leaves the field."""
    if blocked.dtype != torch.uint8 or goal.dtype != torch.uint8 or goal.dim() != 3 or tuple(blocked.shape) != tuple(goal.shape[1:]):
        raise ValueError(f'nav_relax: blocked (gy, gx) and goal (G, gy, gx) uint8 expected, got {blocked.dtype} '
                         f'{tuple(blocked.shape)}, {goal.dtype} {tuple(goal.shape)}')
    if goal.device.type != 'cuda' or blocked.device != goal.device:
        raise _lib.PimlHipError(f'nav_relax: GPU tensors on one device expected (piml_amd has no CPU path), got '
                                f'{blocked.device}, {goal.device}')
    G, gy, gx = (int(n) for n in goal.shape)
    blocked, goal = blocked.contiguous(), goal.contiguous()
    if u is None:
        a = torch.full(goal.shape, float('inf'), device=goal.device, dtype=torch.float32)
        a[goal != 0] = 0.0
    else:
        a = _gpu_f32('u', u).clone()
        if tuple(a.shape) != tuple(goal.shape) or a.device != goal.device:
            raise ValueError(f'nav_relax: u {tuple(goal.shape)} on {goal.device} expected, got {tuple(a.shape)} on {a.device}')
    b = torch.empty_like(a)
    changed = torch.zeros(G, device=goal.device, dtype=torch.int32)

    def queue(n):
        with torch.cuda.device(goal.device):
            _lib.check(_lib.lib().piml_nav_relax(_ptr(blocked), _ptr(goal), _ptr(a), _ptr(b), G, gx, gy, int(n), _ptr(changed),
                                                 _stream()), 'piml_nav_relax')
    if launches is not None:
        queue(launches)
        return (b if int(launches) & 1 else a), int(launches) * NAV_STEPS
    steps = 0
    while True:
        changed.zero_()
        queue(NAV_BATCH)
        steps += NAV_BATCH * NAV_STEPS
        if not bool(changed.any().item()):
            return a, steps
        if steps - NAV_BATCH * NAV_STEPS >= gx * gy:         # the steps before this batch were enough, and it still changed
            raise RuntimeError(f'nav_relax: no fixed point after {steps} steps on a {gx} x {gy} grid')


def nav_sight_relax(blocked, goal, launches=None):
    """The any-angle propagation of piml_nav_sight_relax from its start state on device tensors: blocked (gy, gx) uint8, goal
    (G, gy, gx) uint8 -> (w (G, gy, gx) float32 in cell units, parent (G, gy, gx) int32, the number of Jacobi steps queued).
    launches = None: batches of 32 launches of one step until a batch changed nothing (a fixed point: w only decreases);
    RuntimeError if gx gy steps were not enough.  launches = n: exactly n steps, wherever that leaves the planes."""
    if blocked.dtype != torch.uint8 or goal.dtype != torch.uint8 or goal.dim() != 3 or tuple(blocked.shape) != tuple(goal.shape[1:]):
        raise ValueError(f'nav_sight_relax: blocked (gy, gx) and goal (G, gy, gx) uint8 expected, got {blocked.dtype} '
                         f'{tuple(blocked.shape)}, {goal.dtype} {tuple(goal.shape)}')
    if goal.device.type != 'cuda' or blocked.device != goal.device:
        raise _lib.PimlHipError(f'nav_sight_relax: GPU tensors on one device expected (piml_amd has no CPU path), got '
                                f'{blocked.device}, {goal.device}')
    G, gy, gx = (int(n) for n in goal.shape)
    blocked, goal = blocked.contiguous(), goal.contiguous()
    wa = torch.full(goal.shape, float('inf'), device=goal.device, dtype=torch.float32)
    wa[goal != 0] = 0.0
    lin = torch.arange(gy * gx, device=goal.device, dtype=torch.int32).reshape(1, gy, gx).expand(G, gy, gx)
    pa = torch.where(goal != 0, lin, torch.full_like(lin, -1)).contiguous()
    wb, pb = torch.empty_like(wa), torch.empty_like(pa)
    cache = torch.full((G, gy, gx, 8), -1, device=goal.device, dtype=torch.int32)
    changed = torch.zeros(G, device=goal.device, dtype=torch.int32)

    def queue(n):
        with torch.cuda.device(goal.device):
            _lib.check(_lib.lib().piml_nav_sight_relax(_ptr(blocked), _ptr(goal), _ptr(wa), _ptr(pa), _ptr(wb), _ptr(pb),
                                                       _ptr(cache), G, gx, gy, int(n), _ptr(changed), _stream()),
                       'piml_nav_sight_relax')
    if launches is not None:
        queue(launches)
        return (wb, pb, int(launches)) if int(launches) & 1 else (wa, pa, int(launches))
    steps = 0
    while True:
        changed.zero_()
        queue(NAV_SIGHT_BATCH)
        steps += NAV_SIGHT_BATCH
        if not bool(changed.any().item()):
            return wa, pa, steps
        if steps - NAV_SIGHT_BATCH >= gx * gy:               # the steps before this batch were enough, and it still changed
            raise RuntimeError(f'nav_sight_relax: no fixed point after {steps} steps on a {gx} x {gy} grid')


def nav_field(scenario, cell=0.25, clearance=0.3, near=2.0, bounds=None, device='cuda', sight=False):
    """The floor field of a scene of gates, built once per scene: for every gate g of scenario.entries the geodesic distance
    u[g] to the gate's cells over the free cells of nav_grid_host's grid (piml_nav_relax).  A cell is blocked when an
    obstacle point lies within `clearance` of its centre (wall_force's exact float32 dist2 against a wall_grid of cutoff
    `clearance`); the cells that hold a gate's points are forced free.  near (cells): within it of the gate an agent walks
    straight to its own destination point.  sight = True: also the any-angle table of the same mask (nav_sight_relax): the
    field's w, parent, sight_desc and sight_iterations, which nav_direction and scenario_step_mlapm(nav=) then use.
    Returns a NavField."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.PimlHipError(f'nav_field: a GPU device expected (piml_amd has no CPU path), got {dev}')
    clearance = float(clearance)
    if not math.isfinite(clearance) or not clearance > 0:
        raise ValueError(f'nav_field: a finite clearance > 0 expected, got {clearance}')
    if not math.isfinite(float(near)) or float(near) < 0:
        raise ValueError(f'nav_field: a finite near >= 0 (cells) expected, got {near}')
    h = nav_grid_host(scenario, cell, bounds)
    centres = torch.from_numpy(h.centres).to(dev)
    _, _, index = wall_force(centres, wall_grid(scenario.obstacles, cutoff=clearance, device=dev), 0.0, 0.0,
                             return_selection=True)
    goal = torch.from_numpy(h.goal).to(dev)
    blocked = ((index >= 0) & ~(goal != 0).any(0)).to(torch.uint8).contiguous()
    u, steps = nav_relax(blocked, goal)
    if not sight:
        return NavField(u, blocked, goal, h.x0, h.y0, h.cell, near, clearance, steps)
    w, parent, sight_steps = nav_sight_relax(blocked, goal)
    return NavField(u, blocked, goal, h.x0, h.y0, h.cell, near, clearance, steps, w=w, parent=parent,
                    sight_iterations=sight_steps)


def nav_direction(position, gate, destination, field, return_branch=False, sight=None):
    """The desired direction of piml_nav_direction for every row: position (..., 2), gate (...) integers, destination
    (..., 2) -> e (..., 2) unit vectors.  return_branch: also branch (...) int32 (0 straight, 1 bilinear, 2 descent) and
    neighbour (...) int32 (branch 2's neighbour in the order E, W, N, S, NE, NW, SE, SW; -1 otherwise).  In branches 1 and 2
    position + e (one float32 add) is bitwise the point scenario_step_mlapm(..., nav=field) steers an agent there to.
    sight = None: a field with the any-angle table (nav_field(..., sight=True)) is looked up through it
    (piml_nav_direction_sight: branch 3, sight, in front of 1 and 2; neighbour -1); sight = False forces the lookup without
    the table; sight = True raises ValueError for a field without one."""
    if not isinstance(field, NavField):
        raise TypeError(f'field: a nav_field(...) expected, got {type(field).__name__}')
    if sight and field.sight_desc is None:
        raise ValueError('nav_direction: sight=True needs a field with the any-angle table (nav_field(..., sight=True))')
    use_sight = field.sight_desc is not None if sight is None else bool(sight)
    p = _gpu_f32('position', position)
    d = _gpu_f32('destination', destination)
    if p.dim() < 1 or p.shape[-1] != 2 or p.shape != d.shape:
        raise ValueError(f'position and destination: the same (..., 2) expected, got {tuple(p.shape)}, {tuple(d.shape)}')
    if not isinstance(gate, torch.Tensor) or gate.is_floating_point() or tuple(gate.shape) != tuple(p.shape[:-1]):
        raise ValueError(f'gate: an integer tensor {tuple(p.shape[:-1])} expected')
    if field.u.device != p.device or gate.device != p.device or d.device != p.device:
        raise ValueError(f'position on {p.device}, gate on {gate.device}, destination on {d.device}, the field on {field.u.device}')
    g = gate.to(torch.int32).contiguous()
    lead, rows = p.shape[:-1], p.numel() // 2
    e = torch.zeros_like(p)
    branch = torch.zeros(lead, device=p.device, dtype=torch.int32) if return_branch else None
    nb = torch.full(lead, -1, device=p.device, dtype=torch.int32) if return_branch else None
    if rows:                                     # (an empty problem keeps the fills above: the entry launches nothing)
        with torch.cuda.device(p.device):
            if use_sight:
                _lib.check(_lib.lib().piml_nav_direction_sight(_ptr(p), _ptr(g), _ptr(d), rows, ctypes.byref(field.desc),
                                                               ctypes.byref(field.sight_desc), _ptr(e), _ptr(branch), _ptr(nb),
                                                               _stream()), 'piml_nav_direction_sight')
            else:
                _lib.check(_lib.lib().piml_nav_direction(_ptr(p), _ptr(g), _ptr(d), rows, ctypes.byref(field.desc), _ptr(e),
                                                         _ptr(branch), _ptr(nb), _stream()), 'piml_nav_direction')
    return (e, branch, nb) if return_branch else e


# ---- the density-aware floor field (piml_nav_density, piml_nav_cost, piml_nav_relax_cost; csrc/navdensity.hip) ----
NAV_MAX_RADIUS = 8                     # cells: the cost window's radius (navdensity.hip)
NAV_SOLVERS = ('batch', 'active')      # nav_density_law(solver=): nav_relax_cost's batches, or piml_nav_relax_active
NAV_TILE = 32                          # the solvers' output tile side (navcost.hpp)


class NavDensityLaw:
    """nav_density_law's value: kd, rho0, radius (metres), fmax, every (frames), flow and vref (m/s), solver ('batch' or
    'active') and max_launches (None: nav_field_update's default)"""

    def __init__(self, kd, rho0, radius, fmax, every, flow=0.0, vref=1.3, solver='batch', max_launches=None):
        self.kd, self.rho0, self.radius, self.fmax, self.every = kd, rho0, radius, fmax, every
        self.flow, self.vref = flow, vref
        self.solver, self.max_launches = solver, max_launches

    def radius_cells(self, cell):
        """r = round(radius / cell) cells of a grid of side `cell`; ValueError beyond 8"""
        r = int(round(self.radius / float(cell)))
        if r > NAV_MAX_RADIUS:
            raise ValueError(f'nav density law: radius {self.radius} m is {r} cells of {float(cell):g} m, more than '
                             f'{NAV_MAX_RADIUS}')
        return r

    def __repr__(self):
        tail = f', flow={self.flow}, vref={self.vref}' if self.flow else ''
        if self.solver != 'batch':
            tail += f', solver={self.solver!r}' + (f', max_launches={self.max_launches}' if self.max_launches else '')
        return (f'nav_density_law(kd={self.kd}, rho0={self.rho0}, radius={self.radius}, fmax={self.fmax}, '
                f'every={self.every}{tail})')


def nav_density_law(kd, rho0=0.5, radius=0.75, fmax=8.0, every=8, flow=0.0, vref=1.3, solver='batch', max_launches=None):
    """The density term of a floor field: a cell's slowness is f = min(1 + kd max(rho - rho0, 0), fmax), rho (1/m^2) the
    agents counted in the square window of about `radius` metres around the cell (r = round(radius / cell) cells, at most 8)
    over its area, and the field is solved again every `every` frames.  kd (m^2) has no default: as with Aw, Ag and An there
    is no density term unless one is given; kd = 0 is the static field, solved again.  flow > 0: the direction-aware density
    (piml_nav_cost_flow): a counted person weighs 1 - flow (v . d) / vref, d the static field's way to the walker's gate, so
    one walking the walker's way at vref (m/s) weighs 0 and one coming at the walker 1 + flow, and every gate has a cost plane
    of its own; flow = 0 is the head count.  solver: 'batch' solves an update by batches of 16 dense launches with a host
    read after each (nav_relax_cost); 'active' by ONE queue of max_launches launches that step only the tiles that can still
    move (piml_nav_relax_active: the same field bit for bit, no host read, capturable, so `every` may also divide a captured
    run's frames_per_graph).  max_launches (solver='active' only): an even number >= 2; None: twice the launches the static
    solve queued, rounded up to even (nav_field_update) -- a heuristic bound, NavFieldDynamic.check_converged tells when it
    was too small.  ValueError unless kd >= 0, rho0 >= 0, radius >= 0, fmax >= 1, flow >= 0 and vref > 0 are finite, every
    is an integer >= 1, solver is one of the two and max_launches fits it."""
    kd, rho0, radius, fmax = float(kd), float(rho0), float(radius), float(fmax)
    if not all(math.isfinite(x) for x in (kd, rho0, radius, fmax)) or kd < 0 or rho0 < 0 or radius < 0 or fmax < 1:
        raise ValueError(f'nav density law: finite kd >= 0, rho0 >= 0, radius >= 0 and fmax >= 1 expected, got kd={kd}, '
                         f'rho0={rho0}, radius={radius}, fmax={fmax}')
    if isinstance(every, bool) or int(every) != every or int(every) < 1:
        raise ValueError(f'nav density law: every, a whole number of frames >= 1 expected, got {every!r}')
    flow, vref = float(flow), float(vref)
    if not (math.isfinite(flow) and math.isfinite(vref)) or flow < 0 or vref <= 0:
        raise ValueError(f'nav density law: finite flow >= 0 and vref > 0 expected, got flow={flow}, vref={vref}')
    if solver not in NAV_SOLVERS:
        raise ValueError(f"nav density law: solver, one of {', '.join(map(repr, NAV_SOLVERS))} expected, got {solver!r}")
    if max_launches is not None:
        if solver != 'active':
            raise ValueError("nav density law: max_launches belongs to solver='active'")
        if isinstance(max_launches, bool) or int(max_launches) != max_launches or int(max_launches) < 2 or int(max_launches) & 1:
            raise ValueError(f'nav density law: max_launches, an even number of launches >= 2 expected, got {max_launches!r}')
        max_launches = int(max_launches)
    return NavDensityLaw(kd, rho0, radius, fmax, int(every), flow, vref, solver, max_launches)


def _check_density_law(law):
    if not isinstance(law, NavDensityLaw):
        raise TypeError(f'law: a nav_density_law(...) expected, got {type(law).__name__}')


def _base_field(field):
    if not isinstance(field, NavField):
        raise TypeError(f'field: a nav_field(...) expected, got {type(field).__name__}')
    return field


def nav_density(position, mask, field, out=None):
    """The present agents per cell of `field`'s grid (piml_nav_density): position (members, capacity, 2) or (capacity, 2)
    float32, mask (members, capacity) or (capacity), not 0 for a present slot -> count (members, gy, gx) int32 (one member
    for a single run).  An agent's cell is nav_direction's; absent slots, NaN positions and cells outside the grid deposit
    nothing.  out: a count tensor to write in place (it need not be zero)."""
    field = _base_field(field)
    p = _gpu_f32('position', position)
    m = _gpu_f32('mask', mask)
    if p.dim() == 2:
        p, m = p.unsqueeze(0), m.unsqueeze(0)
    if p.dim() != 3 or p.shape[-1] != 2 or tuple(m.shape) != tuple(p.shape[:2]) or p.shape[1] < 1 or p.shape[0] < 1:
        raise ValueError(f'nav_density: position (members, capacity, 2) and mask (members, capacity) expected, got '
                         f'{tuple(p.shape)}, {tuple(m.shape)}')
    if p.device != field.blocked.device or m.device != p.device:
        raise ValueError(f'nav_density: position on {p.device}, mask on {m.device}, the field on {field.blocked.device}')
    M, cap = int(p.shape[0]), int(p.shape[1])
    if out is None:
        out = torch.empty(M, field.gy, field.gx, device=p.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != (M, field.gy, field.gx) or out.device != p.device or not out.is_contiguous():
        raise ValueError(f'nav_density: out, a contiguous int32 {(M, field.gy, field.gx)} tensor on {p.device} expected')
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().piml_nav_density(_ptr(p), _ptr(m), M, cap, field.x0, field.y0, field.cell, field.gx, field.gy,
                                               _ptr(out), _stream()), 'piml_nav_density')
    return out


def nav_cost(count, field, law, out=None):
    """The slowness planes of piml_nav_cost: count (members, gy, gx) int32 of nav_density -> f (members, gy, gx) float32 under
    the nav_density_law `law` on `field`'s grid.  Blocked cells count in the window's area (a known limit)."""
    field = _base_field(field)
    _check_density_law(law)
    r = law.radius_cells(field.cell)
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.dim() != 3 or \
            tuple(count.shape[1:]) != (field.gy, field.gx):
        raise ValueError(f'nav_cost: count, an int32 (members, {field.gy}, {field.gx}) tensor expected')
    if count.device.type != 'cuda' or count.device != field.blocked.device:
        raise _lib.PimlHipError(f'nav_cost: count on the field\'s GPU expected (piml_amd has no CPU path), got {count.device}')
    count = count.contiguous()
    if out is None:
        out = torch.empty(count.shape, device=count.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(count.shape) or out.device != count.device or not out.is_contiguous():
        raise ValueError(f'nav_cost: out, a contiguous float32 {tuple(count.shape)} tensor on {count.device} expected')
    with torch.cuda.device(count.device):
        _lib.check(_lib.lib().piml_nav_cost(_ptr(count), int(count.shape[0]), field.gx, field.gy, field.cell, r, law.kd,
                                            law.rho0, law.fmax, _ptr(out), _stream()), 'piml_nav_cost')
    return out


def _relax_cost(blocked, goal, cost, a, b, changed, launches, gates=False):
    """nav_relax_cost's loop on buffers the caller owns; a holds the start.  gates: cost has a plane per (member, gate)
    (piml_nav_relax_cost_gates).  -> (the buffer with the result, steps)"""
    M, (G, gy, gx) = int(cost.shape[0]), (int(n) for n in goal.shape)
    name = 'piml_nav_relax_cost_gates' if gates else 'piml_nav_relax_cost'

    def queue(n):
        with torch.cuda.device(goal.device):
            _lib.check(getattr(_lib.lib(), name)(_ptr(blocked), _ptr(goal), _ptr(cost), _ptr(a), _ptr(b), M, G, gx, gy,
                                                 int(n), _ptr(changed), _stream()), name)
    if launches is not None:
        queue(launches)
        return (b if int(launches) & 1 else a), int(launches) * NAV_STEPS
    steps = 0
    while True:
        changed.zero_()
        queue(NAV_BATCH)                                     # an even number of launches: the result is in a
        steps += NAV_BATCH * NAV_STEPS
        if not bool(changed.any().item()):
            return a, steps
        if steps - NAV_BATCH * NAV_STEPS >= gx * gy:         # the steps before this batch were enough, and it still changed
            raise RuntimeError(f'nav_relax_cost: no fixed point after {steps} steps on a {gx} x {gy} grid')


def nav_relax_cost(blocked, goal, cost, launches=None):
    """The weighted eikonal solve of piml_nav_relax_cost from the cold start: blocked (gy, gx) uint8 and goal (G, gy, gx)
    uint8 shared by all members, cost (members, gy, gx) float32 >= 1 -> (u (members, G, gy, gx) float32 in cell units, the
    number of Jacobi steps queued).  launches = None: batches of 16 launches of 8 steps until a batch changed nothing in any
    plane (a fixed point: u only decreases from the cold start); RuntimeError if gx gy steps were not enough.  launches = n:
    exactly n launches, wherever that leaves the field."""
    if blocked.dtype != torch.uint8 or goal.dtype != torch.uint8 or goal.dim() != 3 or tuple(blocked.shape) != tuple(goal.shape[1:]):
        raise ValueError(f'nav_relax_cost: blocked (gy, gx) and goal (G, gy, gx) uint8 expected, got {blocked.dtype} '
                         f'{tuple(blocked.shape)}, {goal.dtype} {tuple(goal.shape)}')
    if goal.device.type != 'cuda' or blocked.device != goal.device:
        raise _lib.PimlHipError(f'nav_relax_cost: GPU tensors on one device expected (piml_amd has no CPU path), got '
                                f'{blocked.device}, {goal.device}')
    cost = _gpu_f32('cost', cost)
    if cost.dim() != 3 or tuple(cost.shape[1:]) != tuple(blocked.shape) or cost.shape[0] < 1 or cost.device != goal.device:
        raise ValueError(f'nav_relax_cost: cost (members, {blocked.shape[0]}, {blocked.shape[1]}) on {goal.device} expected, '
                         f'got {tuple(cost.shape)} on {cost.device}')
    M = int(cost.shape[0])
    blocked, goal = blocked.contiguous(), goal.contiguous()
    start = torch.where(goal != 0, 0.0, float('inf')).to(torch.float32)
    a = start.unsqueeze(0).repeat(M, 1, 1, 1).contiguous()
    b = torch.empty_like(a)
    changed = torch.zeros(M * int(goal.shape[0]), device=goal.device, dtype=torch.int32)
    return _relax_cost(blocked, goal, cost, a, b, changed, launches)


# ---- the direction-aware density (piml_nav_descent, piml_nav_flow, piml_nav_cost_flow, piml_nav_relax_cost_gates; csrc/navflow.hip) ----
NAV_FLOW_MAX_CAPACITY = (1 << 18) - 1  # slots: a window sum of momenta stays inside int32 (navflow.hip)


def nav_descent(field, out=None):
    """The way to each gate of piml_nav_descent: d (G, gy, gx, 2) float32, the upwind unit direction of steepest descent of
    `field`'s STATIC u; (0, 0) on goal cells and where u is +inf.  Once per scene, before any capture."""
    field = _base_field(field)
    u = field.base.u if isinstance(field, NavFieldDynamic) else field.u
    if u.device.type != 'cuda':
        raise _lib.PimlHipError(f'nav_descent: a field on a GPU expected (piml_amd has no CPU path), got {u.device}')
    u = u.contiguous()
    shape = (field.G, field.gy, field.gx, 2)
    if out is None:
        out = torch.empty(shape, device=u.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != u.device or not out.is_contiguous():
        raise ValueError(f'nav_descent: out, a contiguous float32 {shape} tensor on {u.device} expected')
    with torch.cuda.device(u.device):
        _lib.check(_lib.lib().piml_nav_descent(_ptr(u), field.G, field.gx, field.gy, _ptr(out), _stream()), 'piml_nav_descent')
    return out


def nav_flow(position, velocity, mask, field, out=None):
    """nav_density with the velocities kept (piml_nav_flow): position, velocity (members, capacity, 2) or (capacity, 2)
    float32, mask (members, capacity) or (capacity) -> (count (members, gy, gx) int32, nav_density's, and mom (members, 2, gy,
    gx) int32: per cell the sum of the counted slots' velocity components in 2^-10 m/s, each clamped to +-8 m/s, rounded half
    to even, 0 when not finite).  out: a (count, mom) pair to write in place (neither need be zero).  ValueError for
    2^18 slots or more."""
    field = _base_field(field)
    p, v, m = _gpu_f32('position', position), _gpu_f32('velocity', velocity), _gpu_f32('mask', mask)
    if p.dim() == 2:
        p, v, m = p.unsqueeze(0), v.unsqueeze(0), m.unsqueeze(0)
    if p.dim() != 3 or p.shape[-1] != 2 or tuple(v.shape) != tuple(p.shape) or tuple(m.shape) != tuple(p.shape[:2]) or \
            p.shape[1] < 1 or p.shape[0] < 1:
        raise ValueError(f'nav_flow: position and velocity (members, capacity, 2) and mask (members, capacity) expected, got '
                         f'{tuple(p.shape)}, {tuple(v.shape)}, {tuple(m.shape)}')
    if p.device != field.blocked.device or m.device != p.device or v.device != p.device:
        raise ValueError(f'nav_flow: position on {p.device}, velocity on {v.device}, mask on {m.device}, the field on '
                         f'{field.blocked.device}')
    M, cap = int(p.shape[0]), int(p.shape[1])
    if cap > NAV_FLOW_MAX_CAPACITY:
        raise ValueError(f'nav_flow: {cap} slots, at most {NAV_FLOW_MAX_CAPACITY} (the momentum sums are int32)')
    shapes = (M, field.gy, field.gx), (M, 2, field.gy, field.gx)
    if out is None:
        out = tuple(torch.empty(sh, device=p.device, dtype=torch.int32) for sh in shapes)
    elif len(out) != 2 or any(o.dtype != torch.int32 or tuple(o.shape) != sh or o.device != p.device or not o.is_contiguous()
                              for o, sh in zip(out, shapes)):
        raise ValueError(f'nav_flow: out, contiguous int32 {shapes[0]} and {shapes[1]} tensors on {p.device} expected')
    count, mom = out
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().piml_nav_flow(_ptr(p), _ptr(v), _ptr(m), M, cap, field.x0, field.y0, field.cell, field.gx,
                                            field.gy, _ptr(count), _ptr(mom), _stream()), 'piml_nav_flow')
    return count, mom


def nav_cost_flow(count, mom, descent, field, law, out=None):
    """The slowness planes per gate of piml_nav_cost_flow: count (members, gy, gx) and mom (members, 2, gy, gx) int32 of
    nav_flow, descent (G, gy, gx, 2) float32 of nav_descent -> f (members, G, gy, gx) float32 under the nav_density_law `law`
    (its flow and vref included) on `field`'s grid.  law.flow == 0: every gate's plane is nav_cost's bit for bit."""
    field = _base_field(field)
    _check_density_law(law)
    r = law.radius_cells(field.cell)
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.dim() != 3 or \
            tuple(count.shape[1:]) != (field.gy, field.gx):
        raise ValueError(f'nav_cost_flow: count, an int32 (members, {field.gy}, {field.gx}) tensor expected')
    M = int(count.shape[0])
    if not isinstance(mom, torch.Tensor) or mom.dtype != torch.int32 or tuple(mom.shape) != (M, 2, field.gy, field.gx):
        raise ValueError(f'nav_cost_flow: mom, an int32 {(M, 2, field.gy, field.gx)} tensor expected')
    if not isinstance(descent, torch.Tensor) or descent.dtype != torch.float32 or \
            tuple(descent.shape) != (field.G, field.gy, field.gx, 2):
        raise ValueError(f'nav_cost_flow: descent, a float32 {(field.G, field.gy, field.gx, 2)} tensor expected')
    dev = field.blocked.device
    if count.device.type != 'cuda' or any(t.device != dev for t in (count, mom, descent)):
        raise _lib.PimlHipError(f'nav_cost_flow: count, mom and descent on the field\'s GPU expected (piml_amd has no CPU '
                                f'path), got {count.device}, {mom.device}, {descent.device}')
    count, mom, descent = count.contiguous(), mom.contiguous(), descent.contiguous()
    shape = (M, field.G, field.gy, field.gx)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
        raise ValueError(f'nav_cost_flow: out, a contiguous float32 {shape} tensor on {dev} expected')
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().piml_nav_cost_flow(_ptr(count), _ptr(mom), _ptr(descent), M, field.G, field.gx, field.gy,
                                                 field.cell, r, law.kd, law.rho0, law.fmax, law.flow, law.vref, _ptr(out),
                                                 _stream()), 'piml_nav_cost_flow')
    return out


def nav_relax_cost_gates(blocked, goal, cost, launches=None):
    """nav_relax_cost with a cost plane per (member, gate) (piml_nav_relax_cost_gates): cost (members, G, gy, gx) float32 >= 1
    -> (u (members, G, gy, gx), the Jacobi steps queued); launches as nav_relax_cost's.  With the same plane for every gate
    of a member it is nav_relax_cost bit for bit."""
    if blocked.dtype != torch.uint8 or goal.dtype != torch.uint8 or goal.dim() != 3 or tuple(blocked.shape) != tuple(goal.shape[1:]):
        raise ValueError(f'nav_relax_cost_gates: blocked (gy, gx) and goal (G, gy, gx) uint8 expected, got {blocked.dtype} '
                         f'{tuple(blocked.shape)}, {goal.dtype} {tuple(goal.shape)}')
    if goal.device.type != 'cuda' or blocked.device != goal.device:
        raise _lib.PimlHipError(f'nav_relax_cost_gates: GPU tensors on one device expected (piml_amd has no CPU path), got '
                                f'{blocked.device}, {goal.device}')
    cost = _gpu_f32('cost', cost)
    if cost.dim() != 4 or tuple(cost.shape[1:]) != tuple(goal.shape) or cost.shape[0] < 1 or cost.device != goal.device:
        raise ValueError(f'nav_relax_cost_gates: cost (members, {", ".join(str(int(n)) for n in goal.shape)}) on {goal.device} '
                         f'expected, got {tuple(cost.shape)} on {cost.device}')
    M = int(cost.shape[0])
    blocked, goal = blocked.contiguous(), goal.contiguous()
    start = torch.where(goal != 0, 0.0, float('inf')).to(torch.float32)
    a = start.unsqueeze(0).repeat(M, 1, 1, 1).contiguous()
    b = torch.empty_like(a)
    changed = torch.zeros(M * int(goal.shape[0]), device=goal.device, dtype=torch.int32)
    return _relax_cost(blocked, goal, cost, a, b, changed, launches, gates=True)


# ---- the solve by active tiles (piml_nav_relax_active; csrc/navactive.hip) ----
def _check_launches(name, launches):
    if isinstance(launches, bool) or int(launches) != launches or int(launches) < 2 or int(launches) & 1:
        raise ValueError(f'{name}: launches, an even number >= 2 expected (the result is in the first buffer), got {launches!r}')
    return int(launches)


def nav_active_buffers(planes, gy, gx, device):
    """the solver's (flags (2, planes, ty, tx), work (planes), stalled (1)) int32, zeroed"""
    ty, tx = (int(gy) + NAV_TILE - 1) // NAV_TILE, (int(gx) + NAV_TILE - 1) // NAV_TILE
    return (torch.zeros(2, int(planes), ty, tx, device=device, dtype=torch.int32),
            torch.zeros(int(planes), device=device, dtype=torch.int32), torch.zeros(1, device=device, dtype=torch.int32))


def _relax_active(blocked, goal, cost, a, b, flags, work, stalled, launches):
    """one call of piml_nav_relax_active on buffers the caller owns; a holds the cold start and gets the result"""
    M, (G, gy, gx) = int(cost.shape[0]), (int(n) for n in goal.shape)
    with torch.cuda.device(goal.device):
        _lib.check(_lib.lib().piml_nav_relax_active(_ptr(blocked), _ptr(goal), _ptr(cost), int(cost.dim() == 4), _ptr(a), _ptr(b),
                                                    M, G, gx, gy, int(launches), _ptr(flags), _ptr(work), _ptr(stalled),
                                                    _stream()), 'piml_nav_relax_active')


def nav_relax_active(blocked, goal, cost, launches):
    """The weighted eikonal solve by active tiles (piml_nav_relax_active) from the cold start: blocked (gy, gx) uint8 and goal
    (G, gy, gx) uint8 shared by all members; cost (members, gy, gx) float32 >= 1, a plane per member (nav_relax_cost's), or
    (members, G, gy, gx), a plane per member and gate (nav_relax_cost_gates'); launches: an even number >= 2, all queued at
    once, no host read.  -> (u (members, G, gy, gx) float32: the dense solvers' field after the same launches bit for bit;
    work (members, G) int32: the tiles each plane stepped, over all launches; stalled (1,) int32: not 0 when the last launch
    still changed a tile, so launches were too few for the fixed point)."""
    launches = _check_launches('nav_relax_active', launches)
    if blocked.dtype != torch.uint8 or goal.dtype != torch.uint8 or goal.dim() != 3 or tuple(blocked.shape) != tuple(goal.shape[1:]):
        raise ValueError(f'nav_relax_active: blocked (gy, gx) and goal (G, gy, gx) uint8 expected, got {blocked.dtype} '
                         f'{tuple(blocked.shape)}, {goal.dtype} {tuple(goal.shape)}')
    if goal.device.type != 'cuda' or blocked.device != goal.device:
        raise _lib.PimlHipError(f'nav_relax_active: GPU tensors on one device expected (piml_amd has no CPU path), got '
                                f'{blocked.device}, {goal.device}')
    cost = _gpu_f32('cost', cost)
    if cost.dim() not in (3, 4) or cost.shape[0] < 1 or cost.device != goal.device or \
            tuple(cost.shape[1:]) != (tuple(blocked.shape) if cost.dim() == 3 else tuple(goal.shape)):
        raise ValueError(f'nav_relax_active: cost (members, {blocked.shape[0]}, {blocked.shape[1]}) or (members, '
                         f'{", ".join(str(int(n)) for n in goal.shape)}) on {goal.device} expected, got {tuple(cost.shape)} on '
                         f'{cost.device}')
    M, G = int(cost.shape[0]), int(goal.shape[0])
    blocked, goal = blocked.contiguous(), goal.contiguous()
    start = torch.where(goal != 0, 0.0, float('inf')).to(torch.float32)
    a = start.unsqueeze(0).repeat(M, 1, 1, 1).contiguous()
    b = torch.empty_like(a)
    flags, work, stalled = nav_active_buffers(M * G, blocked.shape[0], blocked.shape[1], goal.device)
    _relax_active(blocked, goal, cost, a, b, flags, work, stalled, launches)
    return a, work.view(M, G), stalled


class NavFieldDynamic(NavField):
    """A floor field per member, solved again while the scene runs (nav_field_update): it wraps the scene's static NavField
    `base` -- blocked, goal, the grid scalars and near are the base's -- and owns count, cost (members, gy, gx), u
    (members, G, gy, gx) float32, which the frame reads (desc points at it; member_stride = G gy gx elements), the solver's
    second buffer and its changed flags, and flags, work and stalled of the solve by active tiles (a law with
    solver='active').  All are allocated here, once, before any capture, and written in place.  u starts
    as the base's field in every member; iterations is the steps of the last update, updates their number.
    flow = True (a law with flow > 0, the direction-aware density): it also owns mom (members, 2, gy, gx) int32, descent
    (G, gy, gx, 2) float32 -- nav_descent of the base, computed here -- and cost_gates (members, G, gy, gx) float32, the cost
    the solver then reads; cost keeps its meaning, the head-count slowness, and is not written by a flow update.
    ValueError for a base with the any-angle table: that table is a uniform-cost construction."""

    def __init__(self, base, members=1, flow=False):
        if isinstance(base, NavFieldDynamic) or not isinstance(base, NavField):
            raise TypeError(f'nav field: a static nav_field(...) expected, got {type(base).__name__}')
        if base.sight_desc is not None:
            raise ValueError('nav density: the any-angle table is a uniform-cost construction and cannot carry a density '
                             'term (nav=True or a nav_field without sight=True)')
        M = int(members)
        if not 1 <= M <= MAX_MEMBERS or M * base.G > MAX_MEMBERS or M * base.G * base.gy * base.gx > 2 ** 31 - 1:
            raise ValueError(f'nav density: {M} members x {base.G} gates on a {base.gx} x {base.gy} grid: at most '
                             f'{MAX_MEMBERS} planes and 2^31 - 1 cells')
        self.base, self.members = base, M
        self.blocked, self.goal = base.blocked.contiguous(), base.goal.contiguous()
        self.G, self.gy, self.gx = base.G, base.gy, base.gx
        self.x0, self.y0, self.cell, self.near = base.x0, base.y0, base.cell, base.near
        self.clearance, self.iterations, self.updates = base.clearance, 0, 0
        dev = base.u.device
        self.count = torch.zeros(M, self.gy, self.gx, device=dev, dtype=torch.int32)
        self.cost = torch.ones(M, self.gy, self.gx, device=dev, dtype=torch.float32)
        self.flow = bool(flow)
        self.mom = self.descent = self.cost_gates = None
        if self.flow:
            self.mom = torch.zeros(M, 2, self.gy, self.gx, device=dev, dtype=torch.int32)
            self.descent = nav_descent(base)
            self.cost_gates = torch.ones(M, self.G, self.gy, self.gx, device=dev, dtype=torch.float32)
        self.u = base.u.unsqueeze(0).repeat(M, 1, 1, 1).contiguous()
        self.u_b = torch.empty_like(self.u)
        self.changed = torch.zeros(M * self.G, device=dev, dtype=torch.int32)
        # the solve by active tiles (a law with solver='active'): its flags, work and stalled word; max_launches of the last update
        self.flags, self.work, self.stalled = nav_active_buffers(M * self.G, self.gy, self.gx, dev)
        self.max_launches = 0
        self.start = torch.where(self.goal != 0, 0.0, float('inf')).to(torch.float32).contiguous()      # the cold start
        self.member_stride = self.G * self.gy * self.gx
        d = _lib.NavGrid()
        d.u, d.G, d.gx, d.gy = self.u.data_ptr(), self.G, self.gx, self.gy
        d.x0, d.y0, d.cell, d.near = self.x0, self.y0, self.cell, self.near
        self.desc = d
        self.w = self.parent = self.sight_desc = None
        self.sight_iterations = 0

    def reset(self):
        """every member's u back to the base's static field, in place (the start of a run)"""
        self.u.copy_(self.base.u.unsqueeze(0).expand_as(self.u))
        self.stalled.zero_()
        self.iterations = self.updates = 0

    def default_max_launches(self):
        """the launches of an update under solver='active' when the law names none: twice the launches the static solve
        queued, rounded up to even.  A heuristic bound (a crowd lengthens the quickest paths); check_converged catches it"""
        n = max(2, -(-2 * int(self.base.iterations) // NAV_STEPS))
        return n + (n & 1)

    def check_converged(self):
        """ONE host read of the stalled word of the updates under solver='active' since the last reset: RuntimeError when an
        update's last launch still changed a tile, so its field was not the fixed point"""
        if bool(self.stalled.item()):
            raise RuntimeError(f'nav density: an update of the field had not reached its fixed point after max_launches = '
                               f'{self.max_launches} launches on a {self.gx} x {self.gy} grid: give the law a larger '
                               f"max_launches, or solver='batch'")

    def member(self, m):
        """member m's planes as a static NavField (for nav_direction)"""
        return NavField(self.u[int(m)], self.blocked, self.goal, self.x0, self.y0, self.cell, self.near, self.clearance,
                        self.iterations)

    def to_numpy(self):
        out = super().to_numpy()
        out.count, out.cost, out.members = self.count.cpu().numpy(), self.cost.cpu().numpy(), self.members
        if self.flow:
            out.mom, out.descent, out.cost_gates = (x.cpu().numpy() for x in (self.mom, self.descent, self.cost_gates))
        return out

    def reachable(self, g):
        return self.base.reachable(g)


def nav_field_update(field, st, law):
    """One update of a NavFieldDynamic from the state's present agents: density (st.p, st.mask -> field.count), cost
    (-> field.cost) and a solve FROM THE COLD START into field.u, per member, all in place.  law.flow > 0: the
    direction-aware path on a field built with flow=True (ValueError otherwise): st.p, st.v, st.mask -> field.count and
    field.mom (nav_flow), -> field.cost_gates (nav_cost_flow), and the solve reads a plane per gate.  A warm start is wrong: the
    minimum of the update keeps stale low values where the cost rose.  Batches of 16 launches (an even number, so the result
    is in the buffer the frame reads) until a batch changed nothing: one host read per batch, so this is not capturable and
    runs between replays.  A law with solver='active': the same deposit, cost and cold-start copy, then ONE call of
    piml_nav_relax_active with max_launches launches (the law's, or field.default_max_launches()) -- the same field bit for
    bit when that many launches reach the fixed point, no host read, so the update is capturable; field.work holds the tiles
    each plane stepped, field.stalled is set when the launches were too few (field.check_converged() reads it, once, at the
    end of a run).  Returns the steps queued (also field.iterations)."""
    if not isinstance(field, NavFieldDynamic):
        raise TypeError(f'field: a NavFieldDynamic expected, got {type(field).__name__}')
    _check_density_law(law)
    if field.members != st.seeds.numel():
        raise ValueError(f'nav density: a field of {field.members} members for a state of {st.seeds.numel()}')
    if field.u.device != st.p.device:
        raise ValueError(f'nav field on {field.u.device}, the state on {st.p.device}')
    if law.flow > 0:
        if not field.flow:
            raise ValueError('nav density: a law with flow > 0 needs a field built for it (NavFieldDynamic(base, members, '
                             'flow=True))')
        nav_flow(st.p, st.v, st.mask, field, out=(field.count, field.mom))
        nav_cost_flow(field.count, field.mom, field.descent, field, law, out=field.cost_gates)
    else:
        nav_density(st.p, st.mask, field, out=field.count)
        nav_cost(field.count, field, law, out=field.cost)
    field.u.copy_(field.start.unsqueeze(0).expand_as(field.u))
    if law.solver == 'active':
        n = field.default_max_launches() if law.max_launches is None else _check_launches('nav density law', law.max_launches)
        field.work.zero_()
        _relax_active(field.blocked, field.goal, field.cost_gates if law.flow > 0 else field.cost, field.u, field.u_b, field.flags,
                      field.work, field.stalled, n)
        field.max_launches = n
        field.iterations, field.updates = n * NAV_STEPS, field.updates + 1
        return field.iterations
    u, steps = _relax_cost(field.blocked, field.goal, field.cost_gates if law.flow > 0 else field.cost, field.u, field.u_b,
                           field.changed, None, gates=law.flow > 0)
    assert u is field.u
    field.iterations, field.updates = steps, field.updates + 1
    return steps


class ExitChoiceLaw:
    """exit_choice_law's value: classes (a tuple of tuples of gate indices), margin and commit (metres), every (frames)"""

    def __init__(self, classes, margin, commit, every):
        self.classes, self.margin, self.commit, self.every = classes, margin, commit, every
        self._tables = {}

    def gate_class_host(self, G):
        """the class of each of a scene's G gates as a list of ints, -1 for a gate in no class; ValueError for an index
        outside 0 .. G-1"""
        out = [-1] * int(G)
        for k, cls in enumerate(self.classes):
            for g in cls:
                if not 0 <= g < G:
                    raise ValueError(f'exit choice: gate {g} of class {k} is outside the scene\'s gates 0 .. {int(G) - 1}')
                out[g] = k
        return out

    def gate_class(self, G, device):
        """gate_class_host as a device int32 tensor (made once per scene size and device, before any capture)"""
        key = (int(G), str(torch.device(device)))
        if key not in self._tables:
            self._tables[key] = torch.tensor(self.gate_class_host(G), dtype=torch.int32, device=device)
        return self._tables[key]

    def desc(self, cell):
        """the piml_exit_choice of this law on a grid of side `cell`: margin and commit in cell units, divided in float32"""
        import numpy as np
        d = _lib.ExitChoice()
        with np.errstate(over='ignore'):
            d.margin = float(np.float32(self.margin) / np.float32(cell))
            d.commit = float(np.float32(self.commit) / np.float32(cell))
        d.every = self.every
        return d

    def __repr__(self):
        return (f'exit_choice_law({[list(c) for c in self.classes]}, margin={self.margin}, commit={self.commit}, '
                f'every={self.every})')


def exit_choice_law(classes, margin=1.0, commit=2.0, every=8):
    """The exit choice of a routed scene (piml_nav_choose_exit): `classes` is a list of lists of gate indices, each a set of
    equivalent exits; every `every` frames an agent bound for a gate of a class re-decides among the class's gates (its own
    origin gate excepted) by the floor field's u at its cell -- the walking distance under the static field, a travel-time
    proxy under the density-weighted one -- and switches to the least when that is better by more than `margin` metres,
    unless it is within `commit` metres (of walking distance) of its current gate.  margin = inf never switches from a
    reachable gate.  ValueError for a class of fewer than two gates, a gate in two classes (or twice in one), a negative
    index, margin or commit negative or NaN, every not a whole number >= 1; an index beyond the scene's gates is refused
    when the law meets a scene."""
    try:
        cls = tuple(tuple(int(g) for g in c) for c in classes)
        exact = all(int(g) == g and not isinstance(g, bool) for c in classes for g in c)
    except (TypeError, ValueError):
        raise ValueError(f'exit choice: classes, a list of lists of gate indices expected, got {classes!r}') from None
    if not cls or not exact:
        raise ValueError(f'exit choice: classes, a non-empty list of lists of whole gate indices expected, got {classes!r}')
    seen = set()
    for k, c in enumerate(cls):
        if len(c) < 2:
            raise ValueError(f'exit choice: class {k} has {len(c)} gates: at least two expected')
        for g in c:
            if g < 0:
                raise ValueError(f'exit choice: gate index {g} of class {k} is negative')
            if g in seen:
                raise ValueError(f'exit choice: gate {g} is in two classes (or twice in class {k})')
            seen.add(g)
    margin, commit = float(margin), float(commit)
    if not margin >= 0 or not commit >= 0:
        raise ValueError(f'exit choice: margin >= 0 and commit >= 0 (metres) expected, got {margin}, {commit}')
    if isinstance(every, bool) or int(every) != every or int(every) < 1:
        raise ValueError(f'exit choice: every, a whole number of frames >= 1 expected, got {every!r}')
    return ExitChoiceLaw(cls, margin, commit, int(every))


def resolve_exit_choice(scenario, exit_choice, nav):
    """The exit_choice= argument of the simulate_* methods against their scene and nav= (False already None): None for None or
    False; True -> exit_choice_law(scenario.exit_classes); an ExitChoiceLaw as it is, checked against the scene's gates.
    TypeError for anything else; ValueError without a floor field, for a scene the field cannot route, for True on a scene
    without exit_classes, or for a gate index beyond the scene's gates."""
    if exit_choice is None or exit_choice is False:
        return None
    if exit_choice is not True and not isinstance(exit_choice, ExitChoiceLaw):
        raise TypeError(f'exit_choice: True or an ops_scenario.exit_choice_law(...) expected, got {type(exit_choice).__name__}')
    if nav is None:
        raise ValueError('exit_choice: the choice reads the floor field and needs nav (--nav / --route)')
    check_nav_scene(scenario)
    if exit_choice is True:
        if not getattr(scenario, 'exit_classes', None):
            raise ValueError('exit_choice=True: the scene has no exit_classes (floorplan_scenario(..., exits=[[1, 2], ...]), '
                             'the plan\'s "exits", or an exit_choice_law(classes))')
        exit_choice = exit_choice_law(scenario.exit_classes)
    exit_choice.gate_class_host(scenario.entries.shape[0])
    return exit_choice


def scenario_exit_switches(st):
    """The exit choice's per-slot switch counts of st ((S,) capacity int32), allocated as zeros when first needed and kept
    (scenario_state_reset zeroes them in place)."""
    if getattr(st, 'exit_switches', None) is None:
        st.exit_switches = torch.zeros_like(st.flag)
    return st.exit_switches


def nav_choose_exit(st, field, law, switch_count=None, frame_offset=0):
    """One launch of piml_nav_choose_exit on a scenario state, in front of a frame: at the counter values t = st.t +
    frame_offset with t >= 1 and (t - 1) % law.every == 0 -- tested on the device, so the call can stand in front of every
    frame, captured ones too -- every present agent bound for a gate of one of law's classes re-decides among that class by
    field.u at its cell and, on a switch, gets the destination the spawn would have given it for the new gate (waypoints
    and exit_idx rows flag .. 1, st.dest).  field: a NavField, with or without the any-angle table (u alone is read), or a
    NavFieldDynamic of the state's members (member m reads its own planes).  law: an exit_choice_law(...).  switch_count:
    None, or an int32 tensor of st.flag's shape that counts each slot's switches (scenario_exit_switches(st)).  The checks
    are scenario_step_mlapm(nav=)'s; ValueError also for a gate of the law beyond the scene's."""
    _check_nav(st, field)
    if not isinstance(law, ExitChoiceLaw):
        raise TypeError(f'law: an exit_choice_law(...) expected, got {type(law).__name__}')
    if int(frame_offset) < 0:
        raise ValueError(f'frame_offset must be >= 0, got {frame_offset}')
    if switch_count is not None:
        if not isinstance(switch_count, torch.Tensor) or switch_count.dtype != torch.int32 or \
                tuple(switch_count.shape) != tuple(st.flag.shape) or switch_count.device != st.p.device or \
                not switch_count.is_contiguous():
            raise ValueError(f'switch_count: a contiguous int32 {tuple(st.flag.shape)} tensor on {st.p.device} expected')
    classes = law.gate_class(field.G, st.p.device)
    desc = law.desc(field.cell)
    stride = field.member_stride if isinstance(field, NavFieldDynamic) else 0
    with torch.cuda.device(st.p.device):
        _lib.check(_lib.lib().piml_nav_choose_exit(
            ctypes.byref(st.desc), st.seeds.numel(), _ptr(st.seeds), ctypes.byref(field.desc), stride, _ptr(classes),
            ctypes.byref(desc), None if switch_count is None else _ptr(switch_count), int(frame_offset), _stream()),
            'piml_nav_choose_exit')


def _noise_arg_is_table(st, noise):
    """scenario_step_mlapm's check of `noise`; True for a table"""
    noise_table = isinstance(noise, torch.Tensor)
    if noise_table:
        if noise.dtype != torch.float32 or tuple(noise.shape) != (st.seeds.numel(), 2) or not noise.is_contiguous():
            raise ValueError(f'noise table: a contiguous float32 ({st.seeds.numel()}, 2) tensor of noise_law_table '
                             f'expected, got {noise.dtype} {tuple(noise.shape)}')
        if noise.device != st.p.device:
            raise ValueError(f'noise table on {noise.device}, the state on {st.p.device}')
    elif not isinstance(noise, _lib.NoiseLaw):
        raise TypeError(f'noise: a noise_law or a noise_law_table expected, got {type(noise).__name__}')
    return noise_table


def check_nav_scene(scenario):
    """ValueError unless `scenario` can be routed by a floor field (piml_scenario_step_mlapm_nav's own refusals, said before
    any state exists): GC's spawn law -- the only one with gates and exit_idx -- without groups, and route_max_iters == 0."""
    if scenario.spawn_law == 'clip_groups':
        raise ValueError('nav: a grouped scene cannot be routed by a floor field (its units follow recorded waypoints)')
    if scenario.spawn_law != 'gc':
        raise ValueError(f"nav: the floor field routes scenes of gates (spawn law 'gc') only, not {scenario.spawn_law!r}: "
                         f'only that law has gates and exit_idx')
    if int(scenario.route_max_iters) != 0:
        raise ValueError(f'nav: route_max_iters must be 0, got {scenario.route_max_iters}: with a detour point the '
                         f"agent's waypoint gate is not its destination gate and it would never arrive "
                         f'(dataclasses.replace(scenario, route_max_iters=0))')


def nav_wants_sight(nav):
    """The nav= argument of MLAPM.simulate_* and SweepRun: True -> False (today's field), 'sight' -> True (the field with the
    any-angle table), a NavField -> whether it has the table; TypeError for anything else."""
    if isinstance(nav, NavField):
        return nav.sight_desc is not None
    if nav is True:
        return False
    if isinstance(nav, str) and nav == 'sight':
        return True
    raise TypeError(f"nav: True, 'sight' or a nav_field(...) expected, got {nav!r}")


def _check_nav(st, nav):
    """scenario_step_mlapm's check of `nav`"""
    if not isinstance(nav, NavField):
        raise TypeError(f'nav: a nav_field(...) expected, got {type(nav).__name__}')
    check_nav_scene(st.scenario)
    if nav.G != st.scenario.entries.shape[0]:
        raise ValueError(f'nav: a field of {nav.G} gates for a scene of {st.scenario.entries.shape[0]}')
    if nav.u.device != st.p.device:
        raise ValueError(f'nav field on {nav.u.device}, the state on {st.p.device}')
    if isinstance(nav, NavFieldDynamic) and nav.members != st.seeds.numel():
        raise ValueError(f'nav density: a field of {nav.members} members for a state of {st.seeds.numel()}')


def scenario_step_mlapm(st, law, frame_offset=0, advance=True, walls=None, groups=None, init=False, noise=None, nav=None):
    """One launch: frame t -> t + 1 of st (single or ensemble state) under the MLAPM law `law` (mlapm_law(...)), t =
    st.t + frame_offset: the force of MLAPM.step from the agents present in frame t's records, v' = v + F dt, p' = p + v' dt
    (src/main_mlapm.py:18-36), a' = F, then the scene's arrivals, exits and spawns as scenario_step.  advance: add 1 to
    st.t afterwards (the kernel reads the counter, never writes it; a captured run of K frames passes offsets 0 .. K-1 and
    advances once by K).  Frame 0's spawn is scenario_step(st, init=True), which does not depend on the law.
    law may instead be a table of mlapm_law_table(...) with one row per member of st (member m steps under row m,
    piml_scenario_step_mlapm_laws); ValueError when it does not hold exactly st.seeds.numel() rows or is on another device.
    walls = (grid, wall): the frame with the wall term (piml_scenario_step_mlapm_walls), F = (MLAPM's force) + W of
    wall_force at the agent's position; grid a wall_grid(...) of the scene's obstacles, wall a wall_law(Aw, Bw) for every
    member or a wall_law_table(...) with one row per member.
    A grouped clip scene (st.groups, scenarios.clip_scenario(groups=)) goes to piml_scenario_step_mlapm_groups in every form
    above; groups = a group_law(Ag, dist) for every member or a group_law_table(...) with one row per member adds the group
    term last, F = (the above) + G of group_force on frame t's records; groups = None: no group term, the units still arrive
    together.  ValueError for groups on a scene without them.
    init = True: the init launch instead (frame st.t gets the scene's n_initial agents; law, walls, groups and frame_offset
    are not read, st.t is not advanced) -- scenario_step(st, init=True) for every scene but a grouped one, whose init launch
    is the new entry's.
    noise = a noise_law(An, noise_tau, dt) for every member or a noise_law_table(...) with one row per member: any of the
    forms above with the fluctuation term (piml_scenario_step_mlapm_noise), F = (the above) + eta', added last; eta lives in
    scenario_noise_state(st), allocated at the first such frame (before any capture: a run's first frame is eager) and
    zeroed by scenario_state_reset.  noise = None takes the entries above, untouched.
    nav = a nav_field(...) of the scene: the frame routed by the floor field (piml_scenario_step_mlapm_nav): every slot
    steers to p + nav_direction(p, the gate of its waypoint, destination) in place of its destination (to the destination
    itself in the lookup's branch 0), with or without walls and noise; everything else is the same frame.  ValueError (check_nav_scene) for a grouped scene, a scene rule
    other than GC's, route_max_iters != 0, or a field of another number of gates.  A field with the any-angle table
    (nav_field(..., sight=True)) goes to piml_scenario_step_mlapm_sight: the lookup with its sight branch, the same frame.
    A NavFieldDynamic (a field per member, nav_field_update) goes to piml_scenario_step_mlapm_navdyn: member m looks its
    directions up in its own planes, the same frame; ValueError when its members are not the state's."""
    grouped = getattr(st, 'groups', None) is not None
    if init:
        if not grouped:
            return scenario_step(st, init=True)
        with torch.cuda.device(st.p.device):
            _lib.check(_lib.lib().piml_scenario_step_mlapm_groups(
                ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds), None, None, None, None, None,
                ctypes.byref(st.groups), None, None, 1, 0, _stream()), 'piml_scenario_step_mlapm_groups')
        return
    if groups is not None and not grouped:
        raise ValueError("groups: the scene has no groups (scenarios.clip_scenario(groups=) makes a 'clip_groups' scene)")
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
    if walls is not None:
        grid, wall = walls
        wall_table = isinstance(wall, torch.Tensor)
        if wall_table:
            if wall.dtype != torch.float32 or tuple(wall.shape) != (st.seeds.numel(), 2) or not wall.is_contiguous():
                raise ValueError(f'wall table: a contiguous float32 ({st.seeds.numel()}, 2) tensor of wall_law_table '
                                 f'expected, got {wall.dtype} {tuple(wall.shape)}')
            if wall.device != st.p.device:
                raise ValueError(f'wall table on {wall.device}, the state on {st.p.device}')
        elif not isinstance(wall, _lib.WallLaw):
            raise TypeError(f'walls: (wall_grid, wall_law or wall_law_table) expected, got {type(wall).__name__}')
        if grid.cell_start.device != st.p.device:
            raise ValueError(f'wall grid on {grid.cell_start.device}, the state on {st.p.device}')
    if nav is not None:
        _check_nav(st, nav)
        grid, wall = walls if walls is not None else (None, None)
        wall_table = isinstance(wall, torch.Tensor)
        na = None
        if noise is not None:
            noise_table = _noise_arg_is_table(st, noise)
            na = _lib.NoiseArgs()
            na.state = scenario_noise_state(st).data_ptr()
            if noise_table:
                na.law_table = noise.data_ptr()
            else:
                na.law = noise
        with torch.cuda.device(st.p.device):
            head = (ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds),
                    None if table else ctypes.byref(law), _ptr(law) if table else None,
                    None if grid is None else ctypes.byref(grid.desc),
                    None if wall is None or wall_table else ctypes.byref(wall), _ptr(wall) if wall_table else None,
                    ctypes.byref(nav.desc))
            tail = (None if na is None else ctypes.byref(na), int(frame_offset), _stream())
            if isinstance(nav, NavFieldDynamic):
                _lib.check(_lib.lib().piml_scenario_step_mlapm_navdyn(*head, nav.member_stride, *tail),
                           'piml_scenario_step_mlapm_navdyn')
            elif nav.sight_desc is not None:
                _lib.check(_lib.lib().piml_scenario_step_mlapm_sight(*head, ctypes.byref(nav.sight_desc), *tail),
                           'piml_scenario_step_mlapm_sight')
            else:
                _lib.check(_lib.lib().piml_scenario_step_mlapm_nav(*head, *tail), 'piml_scenario_step_mlapm_nav')
            if advance:
                st.t.add_(1)
        return
    if noise is not None:
        noise_table = _noise_arg_is_table(st, noise)
        group_table = _group_arg_is_table(st, groups) if grouped else False
        grid, wall = walls if walls is not None else (None, None)
        wall_table = isinstance(wall, torch.Tensor)
        na = _lib.NoiseArgs()
        na.state = scenario_noise_state(st).data_ptr()
        if noise_table:
            na.law_table = noise.data_ptr()
        else:
            na.law = noise
        with torch.cuda.device(st.p.device):
            _lib.check(_lib.lib().piml_scenario_step_mlapm_noise(
                ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds),
                None if table else ctypes.byref(law), _ptr(law) if table else None,
                None if grid is None else ctypes.byref(grid.desc),
                None if wall is None or wall_table else ctypes.byref(wall), _ptr(wall) if wall_table else None,
                ctypes.byref(st.groups) if grouped else None, None if groups is None or group_table else ctypes.byref(groups),
                _ptr(groups) if group_table else None, ctypes.byref(na), 0, int(frame_offset), _stream()),
                'piml_scenario_step_mlapm_noise')
            if advance:
                st.t.add_(1)
        return
    if grouped:
        group_table = _group_arg_is_table(st, groups)
        grid, wall = walls if walls is not None else (None, None)
        wall_table = isinstance(wall, torch.Tensor)
        with torch.cuda.device(st.p.device):
            _lib.check(_lib.lib().piml_scenario_step_mlapm_groups(
                ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds),
                None if table else ctypes.byref(law), _ptr(law) if table else None,
                None if grid is None else ctypes.byref(grid.desc),
                None if wall is None or wall_table else ctypes.byref(wall), _ptr(wall) if wall_table else None,
                ctypes.byref(st.groups), None if groups is None or group_table else ctypes.byref(groups),
                _ptr(groups) if group_table else None, 0, int(frame_offset), _stream()), 'piml_scenario_step_mlapm_groups')
            if advance:
                st.t.add_(1)
        return
    if walls is not None:
        grid, wall = walls
        with torch.cuda.device(st.p.device):
            _lib.check(_lib.lib().piml_scenario_step_mlapm_walls(
                ctypes.byref(st.desc), ctypes.byref(st.rules), st.seeds.numel(), _ptr(st.seeds),
                None if table else ctypes.byref(law), _ptr(law) if table else None, ctypes.byref(grid.desc),
                None if wall_table else ctypes.byref(wall), _ptr(wall) if wall_table else None, int(frame_offset),
                _stream()), 'piml_scenario_step_mlapm_walls')
            if advance:
                st.t.add_(1)
        return
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
