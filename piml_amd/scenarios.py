"""Open-world scenarios: a scene description for `BaseSimulator.simulate_scenario`, its result, and the v2.2 clip writer.

A `Scenario` is data: entry segments sampled as points (agents appear at and leave through them), the polyline agents are
routed around, the obstacle points the features see, the arrival process and the desired-speed law.  `gc_scenario()` is the
reference's Grand Central hall (src/data/scenarios.py:313-401, GC()) tensor for tensor.  The reference's synthetic scenes
(scenarios.py:9-311: crosswalk, four_directional_square, basic_unit1..3) are the same record with a scene rule instead of
entries and a route: a spawn law, an arrival rule, an initial-velocity law, a speed law and an optional second Poisson
stream (`spawn_law`, `arrival_rule`, ...; piml_scenario_rules).  The per-frame work -- integration, arrival, retirement,
Poisson arrivals, recording -- is one HIP launch of scenario_frame_kernel (piml_amd/csrc/scenario.hip), for a single run
and an ensemble alike; `scenario_state_for` / `scenario_result` are every simulator's set-up and result.

`ScenarioEnsemble` is what `BaseSimulator.simulate_ensemble` returns: S simulations of one scene (one per seed) with a
leading member axis, each of them a `ScenarioResult` through `member(m)`.  `ScenarioSweep` is the ensemble of
`MLAPM.simulate_sweep`: candidates x seeds members, every candidate under its own law.

`clip_scenario(raw_data)` makes a scene of any recorded clip: its geometry, the agents of its first frame, and arrivals
resampled from its own tracks (PIML_SPAWN_CLIP: the table of tracks travels in `entries`).

`floorplan_scenario(walls, gates)` / `load_floorplan(path)` write a user's floor plan down as a scene of gates under GC's law,
with no detour route: the way round its walls is the floor field's (ops_scenario.nav_field).

`save_clip` writes a simulation as the reference's `RawData.save_data` does (src/data/data.py:305-341, version v2.2), so
that `RawData.load_trajectory_data` -- here and in the reference -- reads it back as a training clip (`--iter_flag`).
"""
import dataclasses
import math
import types

import numpy as np
import torch

from . import scenes


@dataclasses.dataclass
class Scenario:
    """An entry / exit scene.  Tensors are float32; `to(device)` moves them."""
    entries: torch.Tensor                  # (E, P, 2) sampled entry segments: origins and destinations ('clip': the track table)
    route_polyline: torch.Tensor           # (R, 2) what utils.route routes around
    obstacles: torch.Tensor                # (M, 2) every obstacle point the features see
    rate_per_s: float = 5.0                # Poisson arrivals per second
    time_unit: float = 0.08                # s per frame
    n_initial: int = 20                    # agents of frame 0
    speed_mean: float = 1.34
    speed_var: float = 0.26
    speed_min: float = 0.7
    uniform_desired_speed: bool = False
    spawn_offset: float = 0.8              # + U[0,1)^2 * spawn_offset on the sampled entry point
    route_clearance: float = 2.0           # r moves to the crossing + clearance * normal
    arrival_radius: float = 1.0
    num_waypoints: int = 2                 # D: (route point, destination)
    route_max_iters: int = 16              # device bound on utils.route's loop
    spawn_cap: int = 8                     # bound of the per-frame Poisson draw (inversion cap)
    name: str = ''
    # scene rule (piml_scenario_rules); the defaults are GC's
    spawn_law: str = 'gc'                  # 'gc', 'crosswalk', 'square', 'unit1', 'unit2', 'unit3', 'clip', 'clip_groups'
    arrival_rule: str = 'gc'               # 'gc', 'radius' |p - dest| < r, 'x_band' |p.x - dest.x| < r, 'x_exit' x > length
    initial_velocity: bool = False         # spawn with velocity heading * v0 (else 0)
    speed_clamp: bool = True               # v0 = max(speed_min, ...) of a normal draw
    fixed_spawn_rate: float = None         # arrivals per frame whatever time_unit (the crosswalk's 5 * 0.08)
    rate2_per_s: float = 0.0               # second Poisson stream (basic_unit3's group 2)
    spawn_cap2: int = 0
    length: float = 0.0                    # scene size (the square: block length)
    width: float = 0.0
    side_ratio: float = 0.0                # basic_unit2
    direction_ratio: float = 0.0
    square_grid: torch.Tensor = None       # the square's (d,) grid coordinates
    # 'clip_groups' (clip_scenario(groups=)): the table's rows bundled into units whose members appear together
    row_unit: torch.Tensor = None          # (E, 2) int32 per table row: its index inside its unit, the unit's size
    unit_rows: torch.Tensor = None         # (Ua,) int32 the first row of each arrival unit
    # exit choice (ops_scenario.exit_choice_law): classes of equivalent exits, a list of lists of gate indices, or None
    exit_classes: list = None

    def to(self, device):
        out = dataclasses.replace(self)
        for f in ('entries', 'route_polyline', 'obstacles'):
            setattr(out, f, getattr(self, f).to(device).contiguous())
        for f in ('row_unit', 'unit_rows'):
            if getattr(self, f) is not None:
                setattr(out, f, getattr(self, f).to(device=device, dtype=torch.int32).contiguous())
        return out

    @property
    def spawn_rate(self):
        """Expected arrivals per frame (the reference's 5 * 0.08)."""
        if self.fixed_spawn_rate is not None:
            return self.fixed_spawn_rate
        return self.rate_per_s * self.time_unit

    @property
    def spawn_rate2(self):
        """Expected arrivals per frame of the second stream."""
        return self.rate2_per_s * self.time_unit if self.spawn_cap2 else 0.0

    def poisson_thresholds(self):
        """ceil(2^24 P(K <= j)), j < spawn_cap, K ~ Poisson(spawn_rate): the spawn count of a frame is the number of these
        its 24-bit uniform reaches (inversion, capped at spawn_cap)."""
        return _poisson_thresholds(self.spawn_rate, self.spawn_cap)

    def poisson_thresholds2(self):
        """The second stream's thresholds (spawn_rate2, spawn_cap2)."""
        return _poisson_thresholds(self.spawn_rate2, self.spawn_cap2)


def _poisson_thresholds(lam, cap):
    p = math.exp(-lam)
    cdf, out = p, []
    for j in range(cap):
        out.append(min(1 << 24, math.ceil(cdf * (1 << 24))))
        p *= lam / (j + 1)
        cdf += p
    return out


def gc_scenario(time_unit=0.08, uniform_desired_speed=False):
    """The Grand Central hall of the reference (scenarios.py:313-366): the wall polyline resampled per edge with
    torch.linspace(a, b, int(len / 0.05)) (3994 points), the 100-point pillar (what agents are routed around) and the 7
    entries of 100 points each, bit for bit.  obstacles = wall + pillar."""
    wall_node = torch.tensor(scenes._WALL_NODES.tolist(), dtype=torch.float32)
    wall_length = torch.linalg.norm(torch.diff(wall_node, dim=0), dim=1)
    wall = []
    for k in range(wall_node.shape[0] - 1):
        n = int(wall_length[k] / 0.05)
        wall.append(torch.stack((torch.linspace(wall_node[k, 0], wall_node[k + 1, 0], n),
                                 torch.linspace(wall_node[k, 1], wall_node[k + 1, 1], n)), dim=1))
    wall = torch.concat(wall, dim=0)
    theta = torch.linspace(0, 2 * np.pi, 100)
    pillar = torch.stack((scenes.DISC_R * torch.cos(theta) + scenes.DISC_C[0],
                          scenes.DISC_R * torch.sin(theta) + scenes.DISC_C[1]), dim=1)
    z, c = torch.zeros(100), torch.ones(100)
    entries = torch.stack([
        torch.stack((z, torch.linspace(5.63 + 1, 16.01 - 1, 100)), dim=1),         # left
        torch.stack((torch.linspace(0 + 1, 5.93 - 1, 100), 35 * c), dim=1),        # top (1)
        torch.stack((torch.linspace(21.43 + 1, 30 - 1, 100), 35 * c), dim=1),      # top (2)
        torch.stack((30 * c, torch.linspace(29.48 + 1, 35 - 1, 100)), dim=1),      # right (1)
        torch.stack((30 * c, torch.linspace(18.99 + 1, 25.62 - 1, 100)), dim=1),   # right (2)
        torch.stack((30 * c, torch.linspace(7.07 + 1, 14.79 - 1, 100)), dim=1),    # right (3)
        torch.stack((torch.linspace(0 + 1, 30 - 1, 100), z), dim=1),               # bottom
    ])
    return Scenario(entries=entries, route_polyline=pillar, obstacles=torch.concat((wall, pillar), dim=0).contiguous(),
                    time_unit=time_unit, uniform_desired_speed=uniform_desired_speed, name='gc')


FLOORPLAN_FIELDS = ('rate_per_s', 'n_initial', 'gate_points', 'wall_spacing', 'time_unit', 'speed_mean', 'speed_var',
                    'speed_min', 'uniform_desired_speed', 'spawn_offset', 'arrival_radius', 'spawn_cap', 'name')


def _sample_segment(a, b, n):
    return torch.stack((torch.linspace(float(a[0]), float(b[0]), n), torch.linspace(float(a[1]), float(b[1]), n)), dim=1)


def floorplan_scenario(walls, gates, rate_per_s=5.0, n_initial=20, gate_points=100, wall_spacing=0.05, exits=None,
                       **scenario_fields):
    """A user's floor plan as a scene of gates under GC's law: walls, a list of polylines (each a list of >= 2 (x, y) points,
    resampled per edge at most wall_spacing metres apart into the obstacle points), and gates, a list of 2 .. 64 segments ((ax, ay),
    (bx, by)), each sampled into gate_points points -- the origins and destinations the arrivals are drawn from, GC's
    `entries`.  route_max_iters is 0: the route is the destination itself and the way around the walls is the floor field's
    (ops_scenario.nav_field; MLAPM.simulate_scenario(..., nav=True)); route_polyline is a two-point dummy that is never
    read.  exits: None or the scene's classes of equivalent exits, a list of lists of gate indices (each of two or more,
    no gate in two), kept as Scenario.exit_classes for MLAPM.simulate_scenario(..., exit_choice=True).  scenario_fields: further Scenario fields (time_unit, arrival_radius, spawn_offset, ...).  ValueError on a plan
    that is not of that shape or a field the scene rule owns."""
    def points(x, what, least):
        try:
            t = torch.tensor(x, dtype=torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f'floorplan: {what}: a list of (x, y) points expected') from None
        if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < least or not bool(torch.isfinite(t).all()):
            raise ValueError(f'floorplan: {what}: at least {least} finite (x, y) points expected, got shape {tuple(t.shape)}')
        return t
    owned = {'entries', 'route_polyline', 'obstacles', 'route_max_iters', 'spawn_law', 'arrival_rule', 'num_waypoints',
             'exit_classes'}
    known = {f.name for f in dataclasses.fields(Scenario)}
    bad = sorted(k for k in scenario_fields if k in owned or k not in known)
    if bad:
        raise ValueError(f'floorplan: {bad} are not fields a floor plan may set')
    if not isinstance(gates, (list, tuple)) or not 2 <= len(gates) <= 64:
        raise ValueError(f'floorplan: 2 .. 64 gates expected, got {len(gates) if isinstance(gates, (list, tuple)) else gates!r}')
    if not isinstance(walls, (list, tuple)):
        raise ValueError('floorplan: walls: a list of polylines expected')
    if exits is not None:
        from . import ops_scenario
        try:
            law = ops_scenario.exit_choice_law(exits)
            law.gate_class_host(len(gates))
        except ValueError as ex:
            raise ValueError(f'floorplan: exits: {ex}') from None
        exits = [list(c) for c in law.classes]
    gate_points, wall_spacing = int(gate_points), float(wall_spacing)
    if gate_points < 1 or not math.isfinite(wall_spacing) or not wall_spacing > 0:
        raise ValueError(f'floorplan: gate_points >= 1 and wall_spacing > 0 expected, got {gate_points}, {wall_spacing}')
    entries = []
    for k, gate in enumerate(gates):
        g = points(gate, f'gate {k}', 2)
        if g.shape[0] != 2:
            raise ValueError(f'floorplan: gate {k}: a segment of two points expected, got {g.shape[0]}')
        entries.append(_sample_segment(g[0], g[1], gate_points))
    obstacles = []
    for k, wall in enumerate(walls):
        w = points(wall, f'wall {k}', 2)
        for a, b in zip(w[:-1], w[1:]):
            obstacles.append(_sample_segment(a, b, max(2, math.ceil(float(torch.linalg.norm(b - a)) / wall_spacing) + 1)))
    obstacles = torch.concat(obstacles, dim=0).contiguous() if obstacles else torch.zeros(0, 2)
    fields = dict(name='floorplan', **scenario_fields) if 'name' not in scenario_fields else dict(scenario_fields)
    return Scenario(entries=torch.stack(entries).contiguous(), route_polyline=torch.zeros(2, 2), obstacles=obstacles,
                    rate_per_s=float(rate_per_s), n_initial=int(n_initial), route_max_iters=0, exit_classes=exits, **fields)


def load_floorplan(path):
    """floorplan_scenario of a JSON file: {"walls": [[[x, y], ...], ...], "gates": [[[ax, ay], [bx, by]], ...]} and, optionally,
    "exits": [[1, 2], ...] (floorplan_scenario's exits) and any of FLOORPLAN_FIELDS.  ValueError on anything else."""
    import json
    with open(path) as fh:
        got = json.load(fh)
    if not isinstance(got, dict) or 'walls' not in got or 'gates' not in got:
        raise ValueError(f"{path}: a JSON object with 'walls' and 'gates' expected")
    unknown = sorted(set(got) - {'walls', 'gates', 'exits', *FLOORPLAN_FIELDS})
    if unknown:
        raise ValueError(f"{path}: unknown keys {unknown} (expected walls, gates, exits and {list(FLOORPLAN_FIELDS)})")
    try:
        return floorplan_scenario(got['walls'], got['gates'], **{k: v for k, v in got.items() if k not in ('walls', 'gates')})
    except (TypeError, ValueError) as ex:
        raise ValueError(f'{path}: {ex}') from None


def _no_geometry():
    return torch.zeros(0, 1, 2), torch.zeros(0, 2), torch.zeros(0, 2)


def crosswalk_scenario(length=20.0, width=7.0, num_ped1=10, num_ped2=10, time_unit=0.08, uniform_desired_speed=False):
    """The reference's crosswalk (scenarios.py:9-85): num_ped1 + num_ped2 agents at frame 0 and Poisson arrivals of
    5 * 0.08 per frame (whatever time_unit: the reference hard-codes it), each on a coin side at |x| = length/2 + 3u,
    y = +-width/2, walking (0, -+v0) across to (-+length/2, +-width/2 by a coin) and then (same x, 3 y).  v0 = 1.34 +
    sqrt(0.26) z without a lower clamp; arrival |p - dest| < 1; no obstacles."""
    entries, poly, obs = _no_geometry()
    return Scenario(entries=entries, route_polyline=poly, obstacles=obs, time_unit=time_unit,
                    n_initial=int(num_ped1) + int(num_ped2), uniform_desired_speed=uniform_desired_speed, num_waypoints=2,
                    spawn_law='crosswalk', arrival_rule='radius', initial_velocity=True, speed_clamp=False,
                    fixed_spawn_rate=5 * 0.08, length=float(length), width=float(width), name='crosswalk')


def square_grid(block_length=20.0, peds_density=5):
    """The (d,) grid coordinates of four_directional_square (scenarios.py:93-94), float32 as torch computes them."""
    d = int(peds_density)
    return torch.arange(1 - d, d + 1, 2) * block_length / 2 / d


def square_layout(scenario, perm=None):
    """(position, destination) (4 d^2, 2) of the square's agents in ordinal order (the four blocks: from the left, the
    right, below, above), destinations of cell c at cell perm[c] (perm = None: unshuffled)."""
    g = scenario.square_grid
    d = g.shape[0]
    gx, gy = torch.meshgrid(g, g, indexing='ij')
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    hx, hy = (gx, gy) if perm is None else (gx[perm], gy[perm])
    L = scenario.length
    pos = [(gx - L, gy), (gx + L, gy), (gx, gy - L), (gx, gy + L)]
    dst = [(hx + L, hy), (hx - L, hy), (hx, hy + L), (hx, hy - L)]
    cat = lambda xs: torch.cat([torch.stack(x, dim=1) for x in xs], dim=0)
    assert cat(pos).shape[0] == 4 * d * d
    return cat(pos), cat(dst)


def four_directional_square_scenario(block_length=20.0, peds_density=5, time_unit=0.08, uniform_desired_speed=True):
    """The reference's four_directional_square (scenarios.py:87-134): 4 d^2 agents at frame 0 on a d x d grid in each of
    four blocks around the origin, each walking to the opposite block, destinations shuffled by one randperm(d^2) shared
    by the four blocks; no arrivals; v0 = 1.34 (+ sqrt(0.26) z, no clamp); arrival |p - dest| < 1; obstacles the
    128-point circle of radius 5.  The reference fixes time_unit at 0.08."""
    angle = torch.linspace(-torch.pi, +torch.pi, 128)
    circle = torch.stack((5 * torch.cos(angle), 5 * torch.sin(angle)), dim=1)
    entries, poly, _ = _no_geometry()
    d = int(peds_density)
    return Scenario(entries=entries, route_polyline=poly, obstacles=circle, time_unit=time_unit, n_initial=4 * d * d,
                    uniform_desired_speed=uniform_desired_speed, num_waypoints=1, spawn_cap=0, spawn_law='square',
                    arrival_rule='radius', initial_velocity=False, speed_clamp=False, length=float(block_length),
                    square_grid=square_grid(block_length, d), name='four_directional_square')


def _basic_unit(law, rule, radius, length, width, time_unit, poisson_lambda, uniform_desired_speed, name, **kw):
    entries, poly, obs = _no_geometry()
    return Scenario(entries=entries, route_polyline=poly, obstacles=obs, rate_per_s=float(poisson_lambda),
                    time_unit=time_unit, n_initial=1, speed_mean=1.14, speed_var=0.1, speed_min=0.8,
                    uniform_desired_speed=uniform_desired_speed, arrival_radius=radius, num_waypoints=1, spawn_law=law,
                    arrival_rule=rule, initial_velocity=True, speed_clamp=True, length=float(length),
                    width=float(width), name=name, **kw)


def basic_unit1_scenario(length=20.0, width=10.0, time_unit=0.08, poisson_lambda=5, during=40, uniform_desired_speed=True):
    """The reference's basic_unit1 (scenarios.py:137-181): one agent at frame 0 and Poisson(poisson_lambda time_unit)
    arrivals at (0, width u) walking (v0, 0) to (length, y + 2u - 1); an agent retires when x > length (no arrival flag);
    v0 = 1.14 (+ sqrt(0.1) z, at least 0.8).  `during` is unused, as in the reference."""
    return _basic_unit('unit1', 'x_exit', 1.0, length, width, time_unit, poisson_lambda, uniform_desired_speed, 'basic_unit1')


def basic_unit2_scenario(length=20.0, width=10.0, time_unit=0.08, poisson_lambda=5, side_ratio=0.3, direction_ratio=0.5,
                         during=40, uniform_desired_speed=True):
    """The reference's basic_unit2 (scenarios.py:183-242): basic_unit1's stream, with a fraction side_ratio of the agents
    in the upper half (y += width/2) and a fraction direction_ratio walking right to left (x = length, y = width - y,
    destination x = 0); arrival |p.x - dest.x| < 0.05.  `during` is unused."""
    return _basic_unit('unit2', 'x_band', 0.05, length, width, time_unit, poisson_lambda, uniform_desired_speed, 'basic_unit2',
                       side_ratio=float(side_ratio), direction_ratio=float(direction_ratio))


def basic_unit3_scenario(length=20.0, width=10.0, time_unit=0.08, poisson_lambda=5, poisson_lambda2=1, during=40,
                         uniform_desired_speed=True):
    """The reference's basic_unit3 (scenarios.py:244-311): basic_unit1's stream (rate poisson_lambda) plus a second one
    (rate poisson_lambda2) from (length u, 0) walking (0, v0) to (x + 2u - 1, width); arrival |p - dest| < 1.  A frame's
    first-stream agents take the lower ordinals.  `during` is unused."""
    return _basic_unit('unit3', 'radius', 1.0, length, width, time_unit, poisson_lambda, uniform_desired_speed, 'basic_unit3',
                       rate2_per_s=float(poisson_lambda2), spawn_cap2=8)


CLIP_MAX_INITIAL = 4096                    # the frame's bound on n_initial
CLIP_MAX_WAYPOINTS = 8                     # ... on D
CLIP_MAX_SPAWN_CAP = 8                     # ... on spawn_cap
CLIP_SPAWN_TAIL = 1e-6                     # the Poisson mass allowed beyond spawn_cap
CLIP_MAX_GROUP = 4                         # members of an arrival unit (a spawn block's waves); larger groups are cut


def _poisson_tail(lam, cap):
    """P(K > cap), K ~ Poisson(lam)."""
    p = math.exp(-lam)
    cdf = p
    for j in range(cap):
        p *= lam / (j + 1)
        cdf += p
    return max(0.0, 1.0 - cdf)


def _clip_units(groups, win, first, a):
    """The units of clip_scenario(groups=): [(tracks ascending, f_u)] for the initial units (f_u == a) and for the arrival
    units, each list ordered by its units' smallest track.  groups: lists of track indices; win (b - a, N) bool presence in
    the window; first (N) each track's first in-window frame."""
    import warnings
    N = win.shape[1]
    seen = win.any(0)
    taken = set()
    checked = []
    for g in groups:
        g = [int(i) for i in g]
        if len(g) < 2:
            raise ValueError(f'clip_scenario: a group of at least 2 tracks expected, got {g}')
        for i in g:
            if not 0 <= i < N:
                raise ValueError(f'clip_scenario: track {i} of group {g} outside the clip\'s 0..{N - 1}')
            if i in taken:
                raise ValueError(f'clip_scenario: track {i} is in two groups (or twice in one)')
            taken.add(i)
        checked.append(sorted(g))
    units, grouped, apart, cut = [], set(), 0, 0
    for g in checked:
        g = [i for i in g if bool(seen[i])]                   # tracks not seen in the window leave their group
        if len(g) < 2:
            continue
        all_on = win[:, g].all(1)
        if not bool(all_on.any()):                            # never all present at once: singles
            apart += 1
            continue
        f_u = a + int(all_on.to(torch.uint8).argmax())
        cut += len(g) > CLIP_MAX_GROUP
        for k in range(0, len(g), CLIP_MAX_GROUP):
            units.append((g[k:k + CLIP_MAX_GROUP], f_u))
        grouped.update(g)
    if apart:
        warnings.warn(f'clip_scenario: {apart} group(s) whose members never share a frame of the window become singles')
    if cut:
        warnings.warn(f'clip_scenario: {cut} group(s) of more than {CLIP_MAX_GROUP} cut into units of at most {CLIP_MAX_GROUP}')
    units += [([i], int(first[i])) for i in seen.nonzero().flatten().tolist() if i not in grouped]
    units.sort(key=lambda u: u[0][0])
    return [u for u in units if u[1] == a], [u for u in units if u[1] != a]


def clip_scenario(raw_data, frames=None, arrival_radius=1.0, jitter=0.0, initial_velocity=True, spawn_cap=8, skip_frames=25,
                  groups=None):
    """A recorded clip as an open-world scene (spawn law 'clip', PIML_SPAWN_CLIP): its obstacles, time unit and D
    waypoints; frame 0 holds the agents present at the window's first frame with the state they had there; afterwards
    agents arrive as a Poisson process at the clip's own rate, each a draw (with replacement) from the tracks that first
    appear later in the window -- origin (+ jitter * U(-1, 1)^2), velocity (0 unless initial_velocity), desired speed and
    the waypoints still ahead of it.  Arrival is |p - dest| < arrival_radius.

    raw_data: a `piml_amd.data.data.RawData` (position, velocity, mask_p, waypoints, dest_idx, obstacles, time_unit).
    frames = (a, b): the window [a, b) of the clip (default: all of it).  The desired speed per agent is
    `data.desired_speed_per_agent(velocity, skip_frames)` over the whole clip, the value the data pipeline feeds the network.
    The table is `entries` (E, 3 + D, 2): per track (position, velocity, (desired_speed, 0), waypoints...), the
    n_initial tracks of the first frame in clip order, then the Ka arrival tracks in clip order; the rate is
    Ka / (b - a - 1) per frame (`fixed_spawn_rate`); no arrival track: spawn_cap 0, a closed scene.
    ValueError: a window shorter than 2 frames or outside the clip, no track in the window, more than 4096 agents in its
    first frame, D > 8, spawn_cap outside 0..8, or P(K > spawn_cap) > 1e-6 at the clip's rate (the frame caps a draw at
    spawn_cap).

    groups (default None: the scene above, law 'clip'): keep the clip's groups as arrival UNITS whose members appear
    together (spawn law 'clip_groups', PIML_SPAWN_CLIP_GROUPS; MLAPM-driven runs only).  A list of lists of track indices
    (columns of raw_data.position; [] is valid: every unit a single), or 'auto' = groupstats.group_stats_of_raw(raw_data,
    frames=frames).groups(0), which needs a GPU.  Tracks not seen in the window leave their group, and a group left with
    one member is a single.  A unit's frame f_u: a single's first in-window frame; a group's first frame of the window at
    which ALL its members are present (none: its members become singles, one warning with the count).  Groups of more than
    CLIP_MAX_GROUP = 4 are cut in ascending track order into consecutive units of at most 4, each at the group's f_u (one
    warning).  A unit with f_u == a is an initial unit, any other an arrival unit, and a track appears in exactly one row:
    a member of an arrival group that was already walking at frame a is therefore NOT in the scene's first frame -- it
    arrives with its group.  Rows: the initial units ordered by their smallest track, members in ascending track order,
    then the arrival units likewise (with groups=[] today's order); a row is (position, velocity, (desired_speed, 0),
    waypoints ahead...) at the unit's f_u.  n_initial is the number of initial rows; `row_unit` (E, 2) int32 holds per row
    (its index inside its unit, the unit's size), `unit_rows` (Ua,) int32 the first row of each arrival unit.  The rate is
    Ua / (b - a - 1) UNITS per frame and the P(K > spawn_cap) check applies to units.
    ValueError besides the above: an index out of range, a track in two groups, a list shorter than 2."""
    from .data.data import desired_speed_per_agent
    pos = torch.as_tensor(raw_data.position).detach().float().cpu()
    vel = torch.as_tensor(raw_data.velocity).detach().float().cpu()
    msk = torch.as_tensor(raw_data.mask_p).detach().cpu() == 1
    way = torch.as_tensor(raw_data.waypoints).detach().float().cpu()
    T, N, D = pos.shape[0], pos.shape[1], way.shape[0]
    a, b = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    if not 0 <= a < b <= T:
        raise ValueError(f'clip_scenario: frames {(a, b)} outside the clip\'s 0..{T}')
    if b - a < 2:
        raise ValueError(f'clip_scenario: a window of at least 2 frames expected, got {(a, b)}')
    if not 1 <= D <= CLIP_MAX_WAYPOINTS:
        raise ValueError(f'clip_scenario: {D} waypoints per agent, 1..{CLIP_MAX_WAYPOINTS} supported')
    if not 0 <= int(spawn_cap) <= CLIP_MAX_SPAWN_CAP:
        raise ValueError(f'clip_scenario: spawn_cap {spawn_cap} outside 0..{CLIP_MAX_SPAWN_CAP} (the device limit)')
    win = msk[a:b]
    seen = win.any(0)
    if not bool(seen.any()):
        raise ValueError(f'clip_scenario: no track in frames {(a, b)}')
    first = a + win.to(torch.uint8).argmax(0)                             # (N) first in-window frame
    if groups is not None:
        if isinstance(groups, str):
            if groups != 'auto':
                raise ValueError(f"clip_scenario: groups: lists of track indices or 'auto' expected, got {groups!r}")
            from .groupstats import group_stats_of_raw
            groups = group_stats_of_raw(raw_data, frames=None if frames is None else (a, b)).groups(0)
        initial, arrivals = _clip_units(list(groups), win, first, a)
        units = initial + arrivals
        order = torch.tensor([i for u, _ in units for i in u], dtype=torch.long)
        f0 = torch.tensor([f for u, f in units for _ in u], dtype=torch.long)
        row_unit = torch.tensor([(q, len(u)) for u, _ in units for q in range(len(u))], dtype=torch.int32).reshape(-1, 2)
        n_initial = sum(len(u) for u, _ in initial)
        Ka = len(arrivals)                                                # arrival UNITS: the rate and the cap count units
        unit_rows = (n_initial + torch.tensor([0] + [len(u) for u, _ in arrivals], dtype=torch.long).cumsum(0)[:-1]).int()
    else:
        order = torch.cat(((seen & (first == a)).nonzero().flatten(), (seen & (first > a)).nonzero().flatten()))
        n_initial = int((seen & (first == a)).sum())
        Ka = order.numel() - n_initial
        f0 = None
    if n_initial > CLIP_MAX_INITIAL:
        raise ValueError(f'clip_scenario: {n_initial} agents in frame {a}, more than {CLIP_MAX_INITIAL}')
    rate = Ka / (b - a - 1)
    cap = int(spawn_cap) if Ka else 0
    if Ka and _poisson_tail(rate, cap) > CLIP_SPAWN_TAIL:
        raise ValueError(f'clip_scenario: {rate:.4g} arrivals per frame: P(K > spawn_cap = {cap}) = '
                         f'{_poisson_tail(rate, cap):.3g} > {CLIP_SPAWN_TAIL:g}; raise spawn_cap (at most '
                         f'{CLIP_MAX_SPAWN_CAP}) or widen the window')
    v0 = desired_speed_per_agent(vel, int(skip_frames))
    if f0 is None:
        f0 = first[order]
    dest_idx = getattr(raw_data, 'dest_idx', None)
    if dest_idx is not None:
        k0 = torch.as_tensor(dest_idx).cpu().long()[f0, order]
    else:                                     # (ScenarioResult.to_raw_data) the waypoint that is the destination there
        d = torch.as_tensor(raw_data.destination).detach().float().cpu()[f0, order]
        k0 = (torch.norm(way[:, order] - d.unsqueeze(0), dim=-1) < 0.01).to(torch.uint8).argmax(0)
    table = torch.full((order.numel(), 3 + D, 2), float('nan'))
    table[:, 0], table[:, 1] = pos[f0, order], vel[f0, order]
    table[:, 2, 0], table[:, 2, 1] = v0[order], 0.0
    q = k0.unsqueeze(1) + torch.arange(D).unsqueeze(0)                    # (E, D) waypoint index of table point 3 + j
    rows = way[:, order].permute(1, 0, 2)                                 # (E, D, 2)
    ahead = torch.gather(rows, 1, q.clamp(max=D - 1).unsqueeze(-1).expand(-1, -1, 2))
    table[:, 3:] = torch.where((q < D).unsqueeze(-1), ahead, torch.full_like(ahead, float('nan')))
    obs = torch.as_tensor(raw_data.obstacles).detach().float().cpu().reshape(-1, 2)
    if groups is not None:
        return Scenario(entries=table.contiguous(), route_polyline=torch.zeros(0, 2), obstacles=obs.contiguous(),
                        time_unit=float(raw_data.time_unit), n_initial=n_initial, spawn_offset=float(jitter),
                        arrival_radius=float(arrival_radius), num_waypoints=D, spawn_cap=cap, spawn_law='clip_groups',
                        arrival_rule='radius', initial_velocity=bool(initial_velocity), speed_clamp=False,
                        fixed_spawn_rate=rate, name='clip', row_unit=row_unit.contiguous(), unit_rows=unit_rows.contiguous())
    return Scenario(entries=table.contiguous(), route_polyline=torch.zeros(0, 2), obstacles=obs.contiguous(),
                    time_unit=float(raw_data.time_unit), n_initial=n_initial, spawn_offset=float(jitter),
                    arrival_radius=float(arrival_radius), num_waypoints=D, spawn_cap=cap, spawn_law='clip',
                    arrival_rule='radius', initial_velocity=bool(initial_velocity), speed_clamp=False,
                    fixed_spawn_rate=rate, name='clip')


SCENARIOS = {'gc': gc_scenario, 'crosswalk': crosswalk_scenario, 'four_directional_square': four_directional_square_scenario,
             'basic_unit1': basic_unit1_scenario, 'basic_unit2': basic_unit2_scenario, 'basic_unit3': basic_unit3_scenario}


def default_capacity(scenario, frames, tail=1e-9):
    """n_initial + the (1 - tail) quantile of Poisson((spawn_rate + spawn_rate2) * (frames - 1)) (at most spawn_cap +
    spawn_cap2 per frame); n_initial for a scene without arrivals.  A grouped clip scene ('clip_groups') draws UNITS: its
    agents are bounded by the unit quantile times the largest arrival-unit size, an upper bound (most units are smaller)."""
    steps = max(int(frames) - 1, 0)
    cap = scenario.spawn_cap + scenario.spawn_cap2
    mu = (scenario.spawn_rate * (scenario.spawn_cap > 0) + scenario.spawn_rate2) * steps
    if mu <= 0 or cap == 0:
        return max(1, scenario.n_initial)
    if mu < 600:
        logp = -mu
        cdf, k = math.exp(logp), 0
        while 1.0 - cdf > tail:
            k += 1
            logp += math.log(mu / k)
            cdf += math.exp(logp)
        q = k
    else:                                     # normal approximation, 6 sigma
        q = int(math.ceil(mu + 6.0 * math.sqrt(mu)))
    largest = 1
    if scenario.unit_rows is not None and scenario.unit_rows.numel():
        largest = int(scenario.row_unit[scenario.unit_rows.long(), 1].max())
    return max(1, scenario.n_initial + min(q, cap * steps) * largest)


def _scene_obstacles(res):
    """the obstacles of a result or ensemble; ValueError when its scene has none"""
    obs = res.obstacles
    if obs is None or obs.numel() == 0:
        raise ValueError('obstacle_stats: the scene has no obstacles')
    return obs


class ScenarioResult(types.SimpleNamespace):
    """What `BaseSimulator.simulate_scenario` returns.  position / velocity / acceleration / destination (T, cap, 2),
    mask_p (T, cap), waypoints (D, cap, 2), desired_speed (cap), obstacles (M, 2), time_unit, spawned (agents generated,
    dropped ones included), dropped (agents past the capacity, never simulated), spawn_count (T) per frame.  Slot n holds
    the agent of ordinal n; slots past min(spawned, cap) never held an agent.  A grouped clip scene's run ('clip_groups')
    also has group_first, group_size (cap) int32 -- per slot the first slot and the size of the unit it was spawned with, 0
    for a slot that never held an agent -- (None for every other scene) and `planted_groups()`.  A scene of gates (GC's law)
    also has exit_gate (cap) int32 -- the gate nearest each slot's destination at the end of the run (row 1 of exit_idx,
    which survives retirement) --, exit_switches (cap) int32, the switches an exit choice made per slot (None without one),
    and `exit_counts()`; exit_gate is None for every other scene."""

    def exit_counts(self):
        """Retired agents per gate: a list of E ints, how many of the slots that held an agent and are absent in the last
        recorded frame were bound for each gate (exit_gate).  ValueError for a scene without gates."""
        return _exit_counts(self.exit_gate, self.mask_p[-1], [self.num_agents], self.num_gates)[0]

    @property
    def num_agents(self):
        return min(int(self.spawned), self.position.shape[1])

    def planted_groups(self):
        """The slot lists of the units of two or more that a grouped clip scene ('clip_groups') spawned together, ordered by
        their first slot (a unit cut by the capacity lists the slots it got); [] for any other scene."""
        gf, gs = getattr(self, 'group_first', None), getattr(self, 'group_size', None)
        if gf is None or gs is None:
            return []
        n = self.num_agents
        gf, gs = gf[:n].detach().cpu().tolist(), gs[:n].detach().cpu().tolist()
        return [list(range(i, min(i + gs[i], n))) for i in range(n) if gf[i] == i and gs[i] >= 2]

    def _dense(self):
        n = self.num_agents
        cpu = lambda x: x.detach().to('cpu')
        return (cpu(self.position[:, :n]), cpu(self.mask_p[:, :n]), cpu(self.waypoints[:, :n]),
                cpu(self.destination[:, :n]), cpu(self.obstacles))

    def to_raw_data(self):
        """A `piml_amd.data.data.RawData` of the simulated agents (CPU tensors; velocity / acceleration as simulated)."""
        from .data.data import RawData
        p, m, w, d, o = self._dense()
        n = p.shape[1]
        raw = RawData(position=p, velocity=self.velocity[:, :n].detach().cpu(),
                      acceleration=self.acceleration[:, :n].detach().cpu(), destination=d, waypoints=w, obstacles=o,
                      mask_p=m, meta_data={'time_unit': float(self.time_unit)})
        raw.num_destinations = w.shape[0]
        raw.mask_v, raw.mask_a = m.clone(), m.clone()          # add_frame's masks (data.py:241-243)
        return raw

    def save_data(self, path):
        p, m, w, d, o = self._dense()
        return save_clip(path, p, m, w, d, o, {'time_unit': float(self.time_unit)})

    def crowd_stats(self, **kw):
        """piml_amd.crowdstats.crowd_stats of the run (simulated velocities; slots past num_agents not swept)."""
        from .crowdstats import crowd_stats
        return crowd_stats(self.position, self.velocity, self.mask_p, n_active=[self.num_agents], **kw)

    def pair_stats(self, **kw):
        """piml_amd.pairstats.pair_stats of the run (simulated velocities; slots past num_agents not swept)."""
        from .pairstats import pair_stats
        return pair_stats(self.position, self.velocity, self.mask_p, n_active=[self.num_agents], **kw)

    def flow_stats(self, **kw):
        """piml_amd.flowstats.flow_stats of the run (simulated velocities; slots past num_agents not swept)."""
        from .flowstats import flow_stats
        return flow_stats(self.position, self.velocity, self.mask_p, n_active=[self.num_agents], **kw)

    def view_stats(self, **kw):
        """piml_amd.viewstats.view_stats of the run (simulated velocities; slots past num_agents not swept)."""
        from .viewstats import view_stats
        return view_stats(self.position, self.velocity, self.mask_p, n_active=[self.num_agents], **kw)

    def track_stats(self, **kw):
        """piml_amd.trackstats.track_stats of the run (positions only, dt = time_unit; slots past num_agents not swept)."""
        from .trackstats import track_stats
        kw.setdefault('dt', float(self.time_unit))
        return track_stats(self.position, self.mask_p, n_active=[self.num_agents], **kw)

    def obstacle_stats(self, **kw):
        """piml_amd.obstaclestats.obstacle_stats of the run against the scene's obstacles (simulated velocities, dt =
        time_unit; slots past num_agents not swept).  ValueError for a scene without obstacles."""
        from .obstaclestats import obstacle_stats
        kw.setdefault('dt', float(self.time_unit))
        return obstacle_stats(self.position, self.velocity, self.mask_p, _scene_obstacles(self), n_active=[self.num_agents],
                              **kw)

    def line_stats(self, lines, **kw):
        """piml_amd.linestats.line_stats of the run against the measurement lines `lines` (L, 4), rows (ax, ay, bx, by)
        (positions only, dt = time_unit; slots past num_agents not swept)."""
        from .linestats import line_stats
        kw.setdefault('dt', float(self.time_unit))
        return line_stats(self.position, self.mask_p, lines, n_active=[self.num_agents], **kw)

    def group_stats(self, **kw):
        """piml_amd.groupstats.group_stats of the run: who walks with whom, group size, spacing and formation (positions
        only, dt = time_unit; slots past num_agents not swept; components='host' | 'device' as group_stats takes it)."""
        from .groupstats import group_stats
        kw.setdefault('dt', float(self.time_unit))
        return group_stats(self.position, self.mask_p, n_active=[self.num_agents], **kw)


def _index(x, key):
    return None if x is None else x[key]


def _exit_counts(exit_gate, last_mask, n_active, num_gates):
    """per member: retired agents per gate.  exit_gate, last_mask (S, cap) or (cap); n_active: a list of S ints"""
    if exit_gate is None or not num_gates:
        raise ValueError('exit_counts: the scene has no gates')
    gate = exit_gate.reshape(len(n_active), -1).detach().cpu()
    mask = last_mask.reshape(len(n_active), -1).detach().cpu()
    out = []
    for m, n in enumerate(n_active):
        gone = gate[m, :n][mask[m, :n] == 0].long()
        out.append(torch.bincount(gone.clamp(0, num_gates - 1), minlength=num_gates).tolist())
    return out


class ScenarioEnsemble(types.SimpleNamespace):
    """What `BaseSimulator.simulate_ensemble` returns: the ScenarioResult fields with a leading member axis -- position /
    velocity / acceleration / destination (S, T, cap, 2), mask_p (S, T, cap), waypoints (S, D, cap, 2), desired_speed
    (S, cap), spawn_count (S, T) -- and seeds, spawned, dropped as lists of S ints; obstacles, time_unit and capacity
    are shared; group_first, group_size (S, cap) for a grouped clip scene, else None.  Member m is the simulation of seed
    seeds[m].  exit_gate, exit_switches (S, cap) and exit_counts() as ScenarioResult's, per member."""

    def exit_counts(self):
        """ScenarioResult.exit_counts of every member: a list of S lists of E ints"""
        cap = self.position.shape[2]
        return _exit_counts(self.exit_gate, self.mask_p[:, -1], [min(int(n), cap) for n in self.spawned], self.num_gates)

    def __len__(self):
        return len(self.seeds)

    def member(self, m):
        """Member m as a ScenarioResult of views (save_data, to_raw_data, num_agents work on it)."""
        return ScenarioResult(
            position=self.position[m], velocity=self.velocity[m], acceleration=self.acceleration[m],
            destination=self.destination[m], mask_p=self.mask_p[m], waypoints=self.waypoints[m],
            desired_speed=self.desired_speed[m], obstacles=self.obstacles, time_unit=self.time_unit,
            spawned=self.spawned[m], dropped=self.dropped[m], spawn_count=self.spawn_count[m], capacity=self.capacity,
            seed=self.seeds[m], group_first=_index(getattr(self, 'group_first', None), m),
            group_size=_index(getattr(self, 'group_size', None), m), exit_gate=_index(getattr(self, 'exit_gate', None), m),
            exit_switches=_index(getattr(self, 'exit_switches', None), m), num_gates=getattr(self, 'num_gates', 0))

    def planted_groups(self, member=0):
        """member(member).planted_groups(): the slot lists of the units of two or more spawned together."""
        return self.member(member).planted_groups()

    def save_data(self, pattern):
        """One v2.2 clip per member at pattern with '{seed}' replaced by the member's seed.  Returns the paths."""
        if '{seed}' not in pattern:
            raise ValueError(f"save_data: the path pattern must contain '{{seed}}', got {pattern!r}")
        return [self.member(m).save_data(pattern.replace('{seed}', str(s))) for m, s in enumerate(self.seeds)]

    def crowd_stats(self, **kw):
        """piml_amd.crowdstats.crowd_stats of every member in one call (member m's slots past its num_agents not swept):
        member m's statistics are bitwise those of member(m).crowd_stats(**kw)."""
        from .crowdstats import crowd_stats
        cap = self.position.shape[2]
        return crowd_stats(self.position, self.velocity, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def pair_stats(self, **kw):
        """piml_amd.pairstats.pair_stats of every member in one call (member m's slots past its num_agents not swept):
        member m's statistics are bitwise those of member(m).pair_stats(**kw)."""
        from .pairstats import pair_stats
        cap = self.position.shape[2]
        return pair_stats(self.position, self.velocity, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def flow_stats(self, **kw):
        """piml_amd.flowstats.flow_stats of every member in one call (member m's slots past its num_agents not swept):
        member m's statistics are bitwise those of member(m).flow_stats(**kw) (axis='auto' is taken over all members: hand
        a member the ensemble's `options['axis']`)."""
        from .flowstats import flow_stats
        cap = self.position.shape[2]
        return flow_stats(self.position, self.velocity, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def view_stats(self, **kw):
        """piml_amd.viewstats.view_stats of every member in one call (member m's slots past its num_agents not swept):
        member m's statistics are bitwise those of member(m).view_stats(**kw)."""
        from .viewstats import view_stats
        cap = self.position.shape[2]
        return view_stats(self.position, self.velocity, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def track_stats(self, **kw):
        """piml_amd.trackstats.track_stats of every member in one call (dt = time_unit; member m's slots past its num_agents
        not swept): member m's statistics are bitwise those of member(m).track_stats(**kw)."""
        from .trackstats import track_stats
        cap = self.position.shape[2]
        kw.setdefault('dt', float(self.time_unit))
        return track_stats(self.position, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def obstacle_stats(self, **kw):
        """piml_amd.obstaclestats.obstacle_stats of every member in one call against the scene's obstacles (dt = time_unit;
        member m's slots past its num_agents not swept): member m's statistics are bitwise those of
        member(m).obstacle_stats(**kw).  ValueError for a scene without obstacles."""
        from .obstaclestats import obstacle_stats
        cap = self.position.shape[2]
        kw.setdefault('dt', float(self.time_unit))
        return obstacle_stats(self.position, self.velocity, self.mask_p, _scene_obstacles(self),
                              n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def line_stats(self, lines, **kw):
        """piml_amd.linestats.line_stats of every member in one call against the measurement lines `lines` (dt = time_unit;
        member m's slots past its num_agents not swept): member m's statistics are bitwise those of
        member(m).line_stats(lines, **kw)."""
        from .linestats import line_stats
        cap = self.position.shape[2]
        kw.setdefault('dt', float(self.time_unit))
        return line_stats(self.position, self.mask_p, lines, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def group_stats(self, **kw):
        """piml_amd.groupstats.group_stats of every member in one call (dt = time_unit; member m's slots past its num_agents
        not swept): member m's statistics are bitwise those of member(m).group_stats(**kw).  components='device' runs the
        link rule and the components of every member in one launch instead of a host loop per member; a
        ScenarioSweep passes it on the same way."""
        from .groupstats import group_stats
        cap = self.position.shape[2]
        kw.setdefault('dt', float(self.time_unit))
        return group_stats(self.position, self.mask_p, n_active=[min(int(n), cap) for n in self.spawned], **kw)

    def collision_counts(self, threshold):
        """Per-member totals of collision_count(member.position, threshold, reduction='sum'): a list of S floats, one
        read-back.  One ops.collision_counts call per member: on a stack of more than 25 frames the count applies the
        friends rule, whose per-pair totals run over the whole stack, so one (S * T, cap, 2) stack would couple members."""
        from . import ops
        thr = (float(threshold),)
        return torch.stack([ops.collision_counts(p, thr)[0].sum() for p in self.position]).tolist()


class ScenarioSweep(ScenarioEnsemble):
    """What `MLAPM.simulate_sweep` returns: a ScenarioEnsemble of n_candidates * seeds_per_candidate members laid out
    candidate-major -- member c * seeds_per_candidate + k ran law params[c] under the k-th seed -- plus params (the
    candidates' dicts), n_candidates and seeds_per_candidate.  `seeds` lists every member's seed (the seed list once per
    candidate); crowd_stats / pair_stats / flow_stats / view_stats / track_stats / obstacle_stats / line_stats / group_stats compute all members in one call, and `.select(sweep.members_of(c)).pooled()` of
    the result pools one candidate."""

    def members_of(self, c):
        """The member indices of candidate c."""
        c = int(c)
        if not 0 <= c < self.n_candidates:
            raise IndexError(f'candidate {c} of {self.n_candidates}')
        return list(range(c * self.seeds_per_candidate, (c + 1) * self.seeds_per_candidate))

    def candidate(self, c):
        """Candidate c's members as a ScenarioEnsemble of views."""
        m = self.members_of(c)
        sl = slice(m[0], m[-1] + 1)
        return ScenarioEnsemble(
            position=self.position[sl], velocity=self.velocity[sl], acceleration=self.acceleration[sl],
            destination=self.destination[sl], mask_p=self.mask_p[sl], waypoints=self.waypoints[sl],
            desired_speed=self.desired_speed[sl], spawn_count=self.spawn_count[sl], obstacles=self.obstacles,
            time_unit=self.time_unit, capacity=self.capacity, seeds=self.seeds[sl], spawned=self.spawned[sl],
            dropped=self.dropped[sl], group_first=_index(getattr(self, 'group_first', None), sl),
            group_size=_index(getattr(self, 'group_size', None), sl), exit_gate=_index(getattr(self, 'exit_gate', None), sl),
            exit_switches=_index(getattr(self, 'exit_switches', None), sl), num_gates=getattr(self, 'num_gates', 0))

    def save_data(self, pattern):
        """One v2.2 clip per member at pattern with '{candidate}' and '{seed}' replaced.  Returns the paths."""
        if '{seed}' not in pattern or '{candidate}' not in pattern:
            raise ValueError(f"save_data: the path pattern must contain '{{candidate}}' and '{{seed}}', got {pattern!r}")
        S = self.seeds_per_candidate
        return [self.member(m).save_data(pattern.replace('{candidate}', str(m // S)).replace('{seed}', str(s)))
                for m, s in enumerate(self.seeds)]


def scenario_state_for(scenario, frames, capacity=None, device='cuda', hist_width=2, **kw):
    """ops_scenario.scenario_state of `scenario` moved to `device`, for `frames` (>= 1) recorded frames and `capacity` slots
    (default: default_capacity); kw: scenario_state's seed / seeds / topk_ped / topk_obs.  The set-up of every simulator's
    simulate_scenario / simulate_ensemble."""
    from . import ops_scenario
    sc = scenario.to(torch.device(device))
    T = int(frames)
    if T < 1:
        raise ValueError(f'frames must be >= 1, got {frames}')
    cap = default_capacity(sc, T) if capacity is None else int(capacity)
    return ops_scenario.scenario_state(sc, cap, T, int(hist_width), **kw)


def scenario_result(st):
    """The ScenarioResult of a finished single-run state of scenario_state_for, or the ScenarioEnsemble of an ensemble's."""
    sc, last = st.scenario, int(st.t.item())
    common = dict(position=st.p_res, velocity=st.v_res, acceleration=st.a_res, destination=st.dest_res, mask_p=st.mask_res,
                  waypoints=st.waypoints, desired_speed=st.desired_speed, obstacles=sc.obstacles, time_unit=sc.time_unit,
                  spawn_count=st.spawn_count, capacity=st.capacity, state=st,
                  group_first=getattr(st, 'group_first', None), group_size=getattr(st, 'group_size', None),
                  exit_gate=st.exit_idx[..., 1, :] if sc.spawn_law == 'gc' else None,
                  exit_switches=getattr(st, 'exit_switches', None), num_gates=sc.entries.shape[0] if sc.spawn_law == 'gc' else 0)
    if st.members is None:
        return ScenarioResult(spawned=int(st.spawned[last & 1].item()), dropped=int(st.dropped.item()), seed=st.seed,
                              **common)
    return ScenarioEnsemble(seeds=st.seed_list, spawned=st.spawned[:, last & 1].tolist(), dropped=st.dropped.tolist(),
                            **common)


def clip_tuple(position, mask_p, waypoints, destination, obstacles, meta_data):
    """(meta_data, trajectories, destinations, obstacles) as RawData.to_trajectories / to_destinations / save_data build
    them (data.py:305-341), vectorised: trajectories[n] = [(x, y, f) for the frames f with mask_p[f, n] == 1];
    destinations = for each agent with at least one, [(wx, wy, t)] for its non-NaN waypoints in order, t = the first frame
    whose destination lies within 0.01 of the waypoint, up to the first waypoint never reached.  Floats are the float32
    values as Python floats."""
    pos = torch.as_tensor(position, dtype=torch.float32).cpu()
    msk = torch.as_tensor(mask_p).cpu()
    way = torch.as_tensor(waypoints, dtype=torch.float32).cpu()
    dst = torch.as_tensor(destination, dtype=torch.float32).cpu()
    T, N = msk.shape[0], msk.shape[1]
    on = (msk == 1).numpy().T                                           # (N, T)
    agent, frame = np.nonzero(on)
    xy = pos.numpy().astype(np.float64)[frame, agent]                   # row-major over (agent, frame)
    rows = list(zip(xy[:, 0].tolist(), xy[:, 1].tolist(), frame.tolist()))
    cuts = np.cumsum(on.sum(1))[:-1].tolist()
    trajectories = [rows[a:b] for a, b in zip([0] + cuts, cuts + [len(rows)])] if N else []
    # first frame each waypoint is the destination (torch.norm's float32 arithmetic, NaN never within reach)
    hit = torch.norm(way.unsqueeze(1) - dst.unsqueeze(0), dim=-1) < 0.01                      # (D, T, N)
    any_hit = hit.any(1).numpy()                                                             # (D, N)
    first = hit.to(torch.uint8).argmax(1).numpy()                                            # (D, N)
    nan = torch.isnan(way).any(-1).numpy()                                                   # (D, N)
    wv = way.numpy().astype(np.float64)
    destinations = []
    for i in range(N):
        des = []
        for k in range(way.shape[0]):
            if nan[k, i]:
                continue
            if not any_hit[k, i]:
                break
            des.append((float(wv[k, i, 0]), float(wv[k, i, 1]), int(first[k, i])))
        if des:
            destinations.append(des)
    meta = dict(meta_data or {})
    meta['version'] = 'v2.2'
    obs = torch.as_tensor(obstacles, dtype=torch.float32).cpu().tolist()
    return meta, trajectories, destinations, obs


def save_clip(path, position, mask_p, waypoints, destination, obstacles, meta_data):
    """RawData.save_data (data.py:335-341): np.save of the v2.2 tuple `clip_tuple` builds.  Returns the path."""
    meta, traj, dest, obs = clip_tuple(position, mask_p, waypoints, destination, obstacles, meta_data)
    np.save(path, np.array((meta, traj, dest, obs), dtype=object))
    return path
