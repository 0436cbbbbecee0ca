"""Open-world scenarios: a scene description for `BaseSimulator.simulate_scenario`, its result, and the v2.2 clip writer.

A `Scenario` is data: entry segments sampled as points (agents appear at and leave through them), the polyline agents are
routed around, the obstacle points the features see, the arrival process and the desired-speed law.  `gc_scenario()` is the
reference's Grand Central hall (src/data/scenarios.py:313-401, GC()) tensor for tensor; other entry / exit scenes (the
crosswalk, basic_unit*) are the same record with other tensors.  The per-frame work -- integration, arrival, retirement,
Poisson arrivals with routing, recording -- is one HIP launch (piml_scenario_step, piml_amd/csrc/scenario.hip).

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
    entries: torch.Tensor                  # (E, P, 2) sampled entry segments: origins and destinations
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

    def to(self, device):
        out = dataclasses.replace(self)
        for f in ('entries', 'route_polyline', 'obstacles'):
            setattr(out, f, getattr(self, f).to(device).contiguous())
        return out

    @property
    def spawn_rate(self):
        """Expected arrivals per frame (the reference's 5 * 0.08)."""
        return self.rate_per_s * self.time_unit

    def poisson_thresholds(self):
        """ceil(2^24 P(K <= j)), j < spawn_cap, K ~ Poisson(spawn_rate): the spawn count of a frame is the number of these
        its 24-bit uniform reaches (inversion, capped at spawn_cap)."""
        lam = self.spawn_rate
        p = math.exp(-lam)
        cdf, out = p, []
        for j in range(self.spawn_cap):
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


SCENARIOS = {'gc': gc_scenario}


def default_capacity(scenario, frames, tail=1e-9):
    """n_initial + the (1 - tail) quantile of Poisson(spawn_rate * (frames - 1)) (at most spawn_cap per frame)."""
    steps = max(int(frames) - 1, 0)
    mu = scenario.spawn_rate * steps
    if mu <= 0:
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
    return max(1, scenario.n_initial + min(q, scenario.spawn_cap * steps))


class ScenarioResult(types.SimpleNamespace):
    """What `BaseSimulator.simulate_scenario` returns.  position / velocity / acceleration / destination (T, cap, 2),
    mask_p (T, cap), waypoints (D, cap, 2), desired_speed (cap), obstacles (M, 2), time_unit, spawned (agents generated,
    dropped ones included), dropped (agents past the capacity, never simulated), spawn_count (T) per frame.  Slot n holds
    the agent of ordinal n; slots past min(spawned, cap) never held an agent."""

    @property
    def num_agents(self):
        return min(int(self.spawned), self.position.shape[1])

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
        return raw

    def save_data(self, path):
        p, m, w, d, o = self._dense()
        return save_clip(path, p, m, w, d, o, {'time_unit': float(self.time_unit)})


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
