"""`MLAPM`: the closed-form social-force law (reference src/models/mlapm.py), same constructor
and `step` signature, evaluated by the HIP pair kernel with an analytic backward.  `simulate_scenario` /
`simulate_ensemble` drive the open-world scenes of piml_amd.scenarios with it (one launch per frame); `simulate_sweep` does
so for a list of laws at once, one law per ensemble member.  With the optional constants Aw, Bw (and wall_cutoff) the scene
runs add a wall term, the repulsion Aw exp(Bw d) of the nearest obstacle point within wall_cutoff (include/piml_hip.h,
piml_scenario_step_mlapm_walls); `step` and `rollout` never have one.  With Ag (and group_dist) the runs of a grouped clip
scene (scenarios.clip_scenario(groups=)) add a group cohesion term, a pull of Ag towards the centroid of the agent's group
(piml_scenario_step_mlapm_groups); `step`, `rollout` and the fits never have one either.  With An (and noise_tau) the scene
runs add a fluctuation term, an Ornstein-Uhlenbeck acceleration per agent of stationary standard deviation An and correlation
time noise_tau (piml_scenario_step_mlapm_noise); again `step`, `rollout` and the gradient fits never have one.  The scene runs
take nav=True | ops_scenario.nav_field(...): the agents of a scene of gates then descend a static floor field instead of
walking the straight line to their destination (piml_scenario_step_mlapm_nav); the field is the scene's, not the law's.
With nav_density=ops_scenario.nav_density_law(kd, ...) as well the field's travel cost grows with the local density and it is
solved again, per member, while the scene runs (piml_scenario_step_mlapm_navdyn).  With exit_choice=True | an
ops_scenario.exit_choice_law(...) routed agents re-decide which gate of a class of equivalent exits they leave through
(piml_nav_choose_exit, one launch in front of every frame)."""
from .. import ops

DEFAULT_WALL_CUTOFF = 2.0     # metres
DEFAULT_GROUP_DIST = 0.5      # metres per further member: Moussaid et al. 2010's (n - 1) / 2
DEFAULT_NOISE_TAU = 0.0       # seconds: white noise


class MLAPM:
    def __init__(self, **args):
        self.args = args
        if args.get('version') not in ops.MLAPM_VARIANTS:
            raise NotImplementedError(args.get('version'))
        wall_args(args)                                       # (ValueError on a half-given or out-of-range wall term)
        group_args(args)                                      # (... or group term)
        noise_args(args)                                      # (... or fluctuation term)

    def step(self, position, velocity, desired_speed, destination, dt, radius=0.3):
        """position, velocity, destination: (N, 2); desired_speed: (N, 1), (N,) or (N, 2).  Returns the new
        velocity `velocity + force * dt` (mlapm.py:10-58).  As in the reference, absent (NaN)
        agents must be filtered out by the caller.  Deviation: version 'UCY' applies the
        one-line `coll.unsqueeze(-1)` fix without which the reference raises for N > 2."""
        a = self.args
        kw = dict(version=a['version'], tau=a['tau'], A=a['A'], B=a['B'], C=a.get('C', 0.0), D=a.get('D', 0.0),
                  theta=a.get('theta', 0.0))
        N = position.shape[0]
        if desired_speed.dim() == 2 and tuple(desired_speed.shape) == (N, 2):
            # the reference's own driver passes (N, 2) (src/main_mlapm.py:13): `desired_speed * ed` then uses a
            # per-component speed.  The kernel takes the x column; the y component's difference is a linear
            # correction of the desired-force term, (0, (v0y - v0x) * ed_y) / tau * dt (exactly zero for equal columns).
            import torch.nn.functional as F
            base = ops.mlapm_step(position, velocity, desired_speed[:, :1], destination, dt, radius, **kw)
            ed_y = F.normalize(destination - position, dim=-1, p=2)[:, 1]
            corr = (desired_speed[:, 1] - desired_speed[:, 0]) * ed_y * (dt / a['tau'])
            return base + F.pad(corr.unsqueeze(-1), (1, 0))
        return ops.mlapm_step(position, velocity, desired_speed, destination, dt, radius, **kw)

    def rollout(self, position, velocity, desired_speed, destination, dt, radius=0.3, steps=200, use_graph=True, fused=True,
                frames_per_graph=8):
        """The simulation loop of src/main_mlapm.py:18-36 on the device: step, explicit Euler
        `p += v dt`, and agents within `radius` of their destination leave the scene (NaN from the next
        frame on).  The reference compacts the active agents on the host every step; here absent
        agents stay in place as NaN rows (`skip_absent`), so shapes are static.  Returns positions and
        velocities (steps + 1, N, 2).
        fused (default): a frame is ONE launch (`ops.mlapm_rollout_step`: the state is read from the trajectory, the frame
        counter lives on the device) and `frames_per_graph` of them are one captured HIP graph; fused=False: the operator
        sequence (MLAPM.step + torch glue, one captured frame replayed)."""
        import torch
        a = self.args
        N = position.shape[0]
        if fused and position.is_cuda:
            spd = desired_speed
            if spd.dim() == 2 and tuple(spd.shape) == (N, 2) and bool((spd[:, 0] == spd[:, 1]).all()):
                spd = spd[:, :1]                              # the reference's driver passes two equal columns (main_mlapm.py:13)
            if spd.numel() == N:
                return self._rollout_fused(position, velocity, spd, destination, dt, radius, steps, use_graph, frames_per_graph)
        p, v = position.clone(), velocity.clone()
        traj_p = torch.full((steps + 1, N, 2), float('nan'), device=p.device)
        traj_v = torch.full((steps + 1, N, 2), float('nan'), device=p.device)
        traj_p[0], traj_v[0] = p, v
        t = torch.ones(1, dtype=torch.long, device=p.device)
        nan = torch.tensor(float('nan'), device=p.device)

        def one():
            v_new = ops.mlapm_step(p, v, desired_speed, destination, dt, radius, version=a['version'], tau=a['tau'],
                                   A=a['A'], B=a['B'], C=a.get('C', 0.0), D=a.get('D', 0.0),
                                   theta=a.get('theta', 0.0), skip_absent=True)
            p_new = p + v_new * dt
            traj_p.index_copy_(0, t, p_new.unsqueeze(0))
            traj_v.index_copy_(0, t, v_new.unsqueeze(0))
            arrived = (torch.norm(p_new - destination, dim=-1, keepdim=True) < radius)
            p.copy_(torch.where(arrived, nan, p_new))
            v.copy_(torch.where(arrived, nan, v_new))
            t.add_(1)
        done = 0
        with torch.no_grad():
            from .. import hip_graphs_safe
            if use_graph and p.is_cuda and steps > 4 and hip_graphs_safe():
                for _ in range(2):
                    one()
                done = 2
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    one()
                for _ in range(steps - done):
                    g.replay()
                done = steps
            for _ in range(steps - done):
                one()
        return traj_p, traj_v

    def _rollout_fused(self, position, velocity, desired_speed, destination, dt, radius, steps, use_graph, frames_per_graph):
        import torch
        a = self.args
        dev, N = position.device, position.shape[0]
        kw = dict(version=a['version'], tau=a['tau'], A=a['A'], B=a['B'], C=a.get('C', 0.0), D=a.get('D', 0.0),
                  theta=a.get('theta', 0.0))
        with torch.no_grad():
            traj_p = torch.full((steps + 1, N, 2), float('nan'), device=dev)
            traj_v = torch.full((steps + 1, N, 2), float('nan'), device=dev)
            traj_p[0], traj_v[0] = position, velocity
            v0 = desired_speed.reshape(N, 1).float().contiguous()
            dest = destination.float().contiguous()
            t = torch.ones(1, dtype=torch.int64, device=dev)
            fin = torch.zeros(1, dtype=torch.int32, device=dev)

            def one():
                ops.mlapm_rollout_step(traj_p, traj_v, v0, dest, t, fin, dt, radius, **kw)
            from .. import hip_graphs_safe
            done = 0
            per = max(1, int(frames_per_graph))
            if use_graph and steps >= 2 * per + 2 and hip_graphs_safe():
                one()                                         # a real frame, also warms the library up
                done = 1
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(per):
                        one()
                for _ in range((steps - done) // per):       # (a launch past the last frame does nothing)
                    g.replay()
                done += (steps - done) // per * per
            for _ in range(steps - done):
                one()
        return traj_p, traj_v

    # ---- open-world scenes (piml_scenario_step_mlapm): the law in place of a PINNSF, same arrivals ----
    def _law(self, radius):
        from .. import ops_scenario
        a = self.args
        return ops_scenario.mlapm_law(a['version'], a['tau'], a['A'], a['B'], a.get('C', 0.0), a.get('D', 0.0),
                                      a.get('theta', 0.0), radius)

    def simulate_scenario(self, scenario, frames, seed=0, capacity=None, use_graph=None, radius=0.3, device='cuda',
                          hist_width=2, frames_per_graph=8, nav=None, nav_density=None, exit_choice=None):
        """Simulate `frames` frames of an entry / exit scene (piml_amd.scenarios: gc_scenario() or a scene of SCENARIOS)
        with this law, as BaseSimulator.simulate_scenario does with a PINNSF: frame 0 spawns the initial agents, every
        further frame is ONE launch -- MLAPM.step's force from the agents present in the frame (main_mlapm.py:18-36),
        v' = v + F dt, p' = p + v' dt, a' = F -- followed by the scene's arrivals, exits and Poisson spawns, which depend
        on (seed, frame, ordinal) only: a PINNSF run of the same seed and capacity sees the same arrivals.
        radius: MLAPM's UCY collision radius (mlapm.py:42-46), NOT the scene's arrival radius.  capacity: default
        scenarios.default_capacity, as the PINNSF path.  use_graph (None: more than 8 frames): `frames_per_graph` frames
        per captured graph, replayed.  hist_width: the velocity history kept for the self_features columns.
        The reference's law has no obstacle or wall term (the square's obstacle points are not felt; GC agents pass the
        pillar by their waypoints), and an agent at rest sees nobody (view is v . r > 0).  MLAPM(..., Aw=, Bw=[,
        wall_cutoff=2.0]) adds one: W = Aw exp(Bw d) (p - q*) / d for the nearest valid obstacle point q* within wall_cutoff,
        isotropic (a resting agent feels it), added to the force last; Aw = 50, Bw = -5 (Helbing and Molnar 1995) is the
        literature's starting point for a fit, not a default.  ValueError when Aw is given and the scene has no obstacles.
        A grouped clip scene (scenarios.clip_scenario(groups=), MLAPM only) spawns its units together whatever the law, and
        the result's group_first / group_size / planted_groups() tell which slots were planted as one.  MLAPM(..., Ag=[,
        group_dist=0.5]) adds the group term last: G = Ag e / |e| towards the centroid c of the agent's present mates, e =
        c - p, once |e| > group_dist (n - 1) -- the attraction term of Moussaid et al. 2010 without their gaze term.  Ag has
        no default; about 3 m/s^2 is the paper's order of magnitude, a starting point for a fit that nobody has verified
        here.  ValueError when Ag is given and the scene has no groups.
        MLAPM(..., An=[, noise_tau=0.0]) adds the fluctuation term of Helbing and Molnar 1995 last, after the wall and group
        terms: an Ornstein-Uhlenbeck acceleration eta per agent, eta' = rho eta + amp z with rho = exp(-dt / noise_tau) and
        amp = An sqrt(1 - rho^2), z two standard normals drawn from (seed, frame, slot) only -- the arrivals do not change and
        a run is still a function of its seed.  An (m/s^2) is the stationary standard deviation of each component and has
        no default; eta is 0 at birth.  With noise_tau = 0 the noise is white, eta = An z: the per-frame acceleration then
        has standard deviation An whatever dt is (a shorter time step does not shrink it).
        nav = True or an ops_scenario.nav_field(...) of the scene: the agents descend a static floor field -- per gate the
        geodesic distance over the free cells of a grid (piml_nav_relax) -- instead of walking the straight line to their
        destination (piml_scenario_step_mlapm_nav), so they go round walls; True builds the field with nav_field's defaults.
        nav = 'sight' builds it with the any-angle table as well (nav_field(sight=True)): the agents then steer along lines
        of sight, at the next turning point of the shortest path (piml_scenario_step_mlapm_sight); a passed field decides by
        whether it has the table.  The field belongs to the scene, not the law.  A scene of gates only (gc_scenario() with
        route_max_iters=0, scenarios.floorplan_scenario): ValueError otherwise (ops_scenario.check_nav_scene).
        nav_density = an ops_scenario.nav_density_law(kd, ...): the floor field's travel cost grows with the local density and
        the field is solved again, per member, every law.every frames from the agents present then (density, cost, a solve
        from the cold start: ops_scenario.nav_field_update; piml_scenario_step_mlapm_navdyn reads it), so routed agents go
        round a congested door.  It needs nav = True or a field without the any-angle table: ValueError otherwise, and in a
        captured run when law.every is not a multiple of frames_per_graph (the update runs between replays).  The field an
        update leaves is read until the next one: it lags by up to law.every frames.  A law with solver='active' solves the
        same field by active tiles with no host read (piml_nav_relax_active), so a captured run also takes an every that
        divides frames_per_graph -- the update is captured with its frames --, and the run raises RuntimeError at its end
        when the law's max_launches were too few for an update's fixed point.
        exit_choice = True or an ops_scenario.exit_choice_law(classes, margin, commit, every): every law.every frames a routed
        agent bound for a gate of a class of equivalent exits re-decides among that class by the field's value at its cell --
        the nearest exit under the static field, the quickest under nav_density's -- and, on a switch, gets the destination
        the spawn would have given it for the new gate (piml_nav_choose_exit: one launch in front of every frame, inside the
        captured graphs too; the schedule is tested on the device).  True takes the scene's exit_classes
        (scenarios.floorplan_scenario(..., exits=)) with the law's defaults.  It needs nav: ValueError otherwise, for a
        grouped scene, and for a gate beyond the scene's.  The result's exit_gate, exit_switches and exit_counts() tell who
        left where.  Without the argument the run is what it was, bit for bit.
        Returns a scenarios.ScenarioResult."""
        return self._simulate(scenario, frames, capacity, use_graph, radius, device, hist_width, frames_per_graph, nav=nav,
                              nav_density=nav_density, exit_choice=exit_choice, seed=seed)

    def simulate_ensemble(self, scenario, frames, seeds, capacity=None, use_graph=None, radius=0.3, device='cuda',
                          hist_width=2, frames_per_graph=8, nav=None, nav_density=None, exit_choice=None):
        """simulate_scenario for every seed of `seeds` in the same launches (grid.y = member; members never see each
        other).  Member m is bitwise simulate_scenario(seed=seeds[m]) with the same capacity; every member shares the
        floor field of nav; with nav_density every member has a field of its own, solved from its own crowd; exit_choice: simulate_scenario's, every member choosing by the field it
        reads.  Returns a scenarios.ScenarioEnsemble."""
        seeds = [int(x) for x in seeds]
        if not seeds:
            raise ValueError('simulate_ensemble: at least one seed expected')
        return self._simulate(scenario, frames, capacity, use_graph, radius, device, hist_width, frames_per_graph, nav=nav,
                              nav_density=nav_density, exit_choice=exit_choice, seeds=seeds)

    def _simulate(self, scenario, frames, capacity, use_graph, radius, device, hist_width, frames_per_graph, nav=None,
                  nav_density=None, exit_choice=None, **state_kw):
        from .. import ops_scenario, scenarios
        law = self._law(radius)
        nav = None if nav is False else nav
        check_nav_density(nav, nav_density)
        exit_choice = ops_scenario.resolve_exit_choice(scenario, exit_choice, nav)
        if nav is not None:
            ops_scenario.nav_wants_sight(nav)
            ops_scenario.check_nav_scene(scenario)
        wall = wall_args(self.args)
        if wall is not None:
            check_scene_walls(scenario)
        group = group_args(self.args)
        if group is not None:
            check_scene_groups(scenario)
        st = scenarios.scenario_state_for(scenario, frames, capacity, device, hist_width, **state_kw)
        walls = None
        if wall is not None:
            walls = (ops_scenario.wall_grid(st.scenario.obstacles, wall[2], st.p.device), ops_scenario.wall_law(*wall[:2]))
        noise = noise_args(self.args)
        if not isinstance(nav, ops_scenario.NavField) and nav is not None:
            nav = ops_scenario.nav_field(st.scenario, device=st.p.device, sight=ops_scenario.nav_wants_sight(nav))
        if nav_density is not None:
            nav_density.radius_cells(nav.cell)
            nav = ops_scenario.NavFieldDynamic(nav, st.seeds.numel(), flow=nav_density.flow > 0)
        self._run_scenario(st, law, use_graph, frames_per_graph, walls=walls,
                           groups=None if group is None else ops_scenario.group_law(*group),
                           noise=None if noise is None else ops_scenario.noise_law(*noise, float(st.scenario.time_unit)),
                           nav=nav, nav_density=nav_density, exit_choice=exit_choice)
        return scenarios.scenario_result(st)

    @staticmethod
    def _run_scenario(st, law, use_graph, frames_per_graph, graph=None, walls=None, groups=None, noise=None, nav=None,
                      nav_density=None, exit_choice=None):
        """frame 0's spawn, then T - 1 MLAPM frames: K = frames_per_graph of them (offsets 0 .. K-1 and one counter add)
        captured into one graph and replayed when use_graph, the rest eagerly.  law: a mlapm_law or a law table; walls:
        None or ops_scenario.scenario_step_mlapm's (grid, wall law or wall table) for the frames with the wall term; groups: None
        or its group law or group table (a grouped clip scene's frames with the group term); noise: None or its noise law or
        noise table (the frames with the fluctuation term; its state is allocated here, before any capture); nav: None or
        the scene's ops_scenario.nav_field (the frames routed by the floor field).  nav_density: None or an
        ops_scenario.nav_density_law, with nav an ops_scenario.NavFieldDynamic of the state's members: the field starts as its
        static base and is updated (ops_scenario.nav_field_update) before the frame at counter value t whenever
        (t - 1) % every == 0 -- a function of the frame counter alone, so eager and captured runs update at the same
        frames; in a captured run that is between replays (a host read per batch of the solve, nothing captured), and every
        must be a multiple of frames_per_graph: ValueError before any launch otherwise.  A law with solver='active' makes no
        host read: an every that is a multiple of frames_per_graph is queued between replays as before, one that divides it
        is captured inside the graph in front of the frames at offsets k with k % every == 0, anything else is the
        ValueError; the run ends with nav.check_converged() (RuntimeError when an update's launches were too few).
        exit_choice: None or an
        ops_scenario.exit_choice_law, with nav: ops_scenario.nav_choose_exit goes in front of every frame, captured ones
        too (its schedule is tested on the device, so it needs no such multiple; where an update falls on the same counter
        value the update runs first and the choice reads the fresh field); st.exit_switches counts the switches.  Returns
        the captured graph (None for an eager run); passed back as `graph` with the same state, the run replays it
        instead of capturing again."""
        import torch
        from .. import ops_scenario, hip_graphs_safe
        steps = st.T - 1
        if use_graph is None:
            use_graph = steps > 8
        per = max(1, int(frames_per_graph))
        inside = False
        if nav_density is not None:
            if not isinstance(nav, ops_scenario.NavFieldDynamic):
                raise TypeError(f'nav_density: nav, an ops_scenario.NavFieldDynamic expected, got {type(nav).__name__}')
            every, active = nav_density.every, nav_density.solver == 'active'
            inside = active and every % per != 0 and per % every == 0      # the update is captured in front of its frames
            if use_graph and steps >= per + 1 and every % per and not inside:
                if active:
                    raise ValueError(f'nav_density: every = {every} frames is neither a multiple of frames_per_graph = {per} '
                                     f'(the update runs between replays) nor a divisor of it (the update is captured with '
                                     f'its frames)')
                raise ValueError(f'nav_density: every = {every} frames is not a multiple of frames_per_graph = '
                                 f"{per}: a captured run updates the field between replays (solver='active' also captures "
                                 f'an update whose every divides frames_per_graph)')

        if exit_choice is not None and nav is None:
            raise ValueError('exit_choice: the choice reads the floor field and needs nav')

        def update(t):                                       # before the frame at counter value t
            if nav_density is not None and t >= 1 and (t - 1) % nav_density.every == 0:
                ops_scenario.nav_field_update(nav, st, nav_density)

        def frame(**kw):                                     # the choice launch, when there is one, then the frame
            if exit_choice is not None:
                ops_scenario.nav_choose_exit(st, nav, exit_choice, st.exit_switches, kw.get('frame_offset', 0))
            ops_scenario.scenario_step_mlapm(st, law, walls=walls, groups=groups, noise=noise, nav=nav, **kw)
        with torch.no_grad():
            if nav_density is not None:
                nav.reset()                                  # frame 0 -> 1 reads the static field
            ops_scenario.scenario_step_mlapm(st, None, init=True)     # frame 0: generate(n_initial)
            if noise is not None:
                ops_scenario.scenario_noise_state(st)
            if exit_choice is not None:
                ops_scenario.scenario_exit_switches(st)      # (allocated before any capture)
            done = 0
            if use_graph and steps >= per + 1 and hip_graphs_safe():
                frame()                                      # a real frame, also warms the library up
                done = 1
                if graph is None:
                    if inside:                               # the update's launches once outside a capture, then the field
                        ops_scenario.nav_field_update(nav, st, nav_density)      # the frames read is put back, in place
                        nav.u.copy_(nav.base.u.unsqueeze(0).expand_as(nav.u))
                        nav.stalled.zero_()
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        for k in range(per):
                            # a replay starts at counter value 1 + j per, so with every dividing per the frame at offset k
                            # is due an update exactly when k % every == 0, in every replay
                            if inside and k % nav_density.every == 0:
                                ops_scenario.nav_field_update(nav, st, nav_density)
                            frame(frame_offset=k, advance=False)
                        st.t.add_(per)
                    if inside:
                        nav.updates = 0                      # (queued so far: none that a replay did not run)
                for j in range((steps - done) // per):
                    if inside:
                        nav.updates += per // nav_density.every
                    else:
                        update(done + j * per)               # (every is a multiple of per: no update falls inside a replay)
                    graph.replay()
                done += (steps - done) // per * per
            for t in range(done, steps):
                update(t)
                frame()
            if nav_density is not None and nav_density.solver == 'active':
                nav.check_converged()                        # the run's one host read of the solver's stalled word
        return graph

    # ---- one law per member (piml_scenario_step_mlapm_laws): a sweep of candidates x seeds in one ensemble run ----
    @staticmethod
    def simulate_sweep(scenario, frames, params, seeds, capacity=None, use_graph=None, radius=0.3, device='cuda',
                       hist_width=2, frames_per_graph=8, wall_cutoff=DEFAULT_WALL_CUTOFF, nav=None, nav_density=None,
                       exit_choice=None):
        """simulate_ensemble for every candidate of `params` in the same launches: params is a list of C dicts in
        MLAPM(**params) form (version, tau, A, B and optionally C, D, theta; an optional 'radius' overrides `radius` for
        that candidate; optionally the wall term's Aw, Bw, in every candidate or in none -- wall_cutoff is common to the
        sweep, a property of the scene's grid; optionally the group term's Ag and group_dist, again in every candidate or
        in none, on a grouped clip scene; optionally the fluctuation term's An and noise_tau, in any subset of the
        candidates: one without An runs without the term, bitwise as if no candidate had one), and member c * len(seeds) + k runs law c under seeds[k] -- candidate-major, every candidate on
        the same seeds and so the same arrivals (common random numbers).  Candidates may differ in version.  Member
        (c, k) is bitwise MLAPM(**params[c]).simulate_ensemble(scenario, frames, seeds, capacity=same)'s member k.
        What the reference does with one process per parameter set (src/utils/grid_search.py) is one run here.
        ValueError: an empty list, an unknown or missing key, candidates with and without a wall term, a wall term in a
        scene without obstacles, candidates with and without a group term, a group term in a scene without groups,
        C * len(seeds) > 65535.  nav: simulate_scenario's; every candidate and seed shares the one field of the scene.
        nav_density: simulate_scenario's; one density law per run, shared by every candidate, and a field per member.
        exit_choice: simulate_scenario's; one law per run, shared by every candidate.
        Returns a scenarios.ScenarioSweep."""
        return SweepRun(scenario, frames, len(params) if hasattr(params, '__len__') else 0, seeds, capacity, use_graph,
                        device, hist_width, frames_per_graph, wall_cutoff, nav, nav_density, exit_choice).run(params, radius)


SWEEP_KEYS = ('version', 'tau', 'A', 'B', 'C', 'D', 'theta', 'radius', 'Aw', 'Bw')
GROUP_KEYS = ('Ag', 'group_dist')       # a candidate's optional group term (a grouped clip scene)
NOISE_KEYS = ('An', 'noise_tau')        # a candidate's optional fluctuation term


def check_nav_density(nav, nav_density):
    """The nav_density= argument of MLAPM.simulate_* and SweepRun against their nav= (False already None): TypeError unless it
    is None or an ops_scenario.nav_density_law; ValueError without a floor field, or with one that has the any-angle table
    (a uniform-cost construction)."""
    from .. import ops_scenario
    if nav_density is None:
        return
    if not isinstance(nav_density, ops_scenario.NavDensityLaw):
        raise TypeError(f'nav_density: an ops_scenario.nav_density_law(...) expected, got {type(nav_density).__name__}')
    if nav is None:
        raise ValueError('nav_density: the density term belongs to the floor field and needs nav=True or a nav_field(...)')
    if ops_scenario.nav_wants_sight(nav):
        raise ValueError('nav_density: the any-angle table is a uniform-cost construction and cannot carry a density term '
                         "(nav=True or a nav_field without sight=True, not 'sight')")
    if isinstance(nav, ops_scenario.NavFieldDynamic):
        raise ValueError('nav_density: nav, the scene\'s static nav_field(...) expected (the run makes its own dynamic field)')


def noise_args(args):
    """(An, noise_tau) of MLAPM(**args)'s fluctuation term, None without one.  ValueError: noise_tau without An, a value that
    is not finite or is negative."""
    import math
    if 'An' not in args:
        if 'noise_tau' in args:
            raise ValueError('MLAPM: noise_tau belongs to the fluctuation term and needs An')
        return None
    An, tau = float(args['An']), float(args.get('noise_tau', DEFAULT_NOISE_TAU))
    if not (math.isfinite(An) and math.isfinite(tau)) or An < 0 or tau < 0:
        raise ValueError(f'MLAPM: finite An >= 0 and noise_tau >= 0 expected, got {An}, {tau}')
    return An, tau


def sweep_noise(params):
    """The (An, noise_tau) pair of every candidate dict -- (0, 0), no term, for a candidate without An --, or None when no
    candidate has a fluctuation term.  Unlike the wall and group terms a sweep may mix candidates with and without one: a
    row of amp 0 is skipped by the frame.  ValueError on a value noise_args refuses."""
    params = list(params)
    rows = [noise_args({k: a[k] for k in NOISE_KEYS if k in a}) for a in params if isinstance(a, dict)]
    if all(r is None for r in rows):
        return None
    return [(0.0, 0.0) if r is None else r for r in rows]


def group_args(args):
    """(Ag, group_dist) of MLAPM(**args)'s group term, None without one.  ValueError: group_dist without Ag, a value that is
    not finite or is negative."""
    import math
    if 'Ag' not in args:
        if 'group_dist' in args:
            raise ValueError('MLAPM: group_dist belongs to the group term and needs Ag')
        return None
    Ag, dist = float(args['Ag']), float(args.get('group_dist', DEFAULT_GROUP_DIST))
    if not (math.isfinite(Ag) and math.isfinite(dist)) or Ag < 0 or dist < 0:
        raise ValueError(f'MLAPM: finite Ag >= 0 and group_dist >= 0 expected, got {Ag}, {dist}')
    return Ag, dist


def check_scene_groups(scenario):
    """ValueError when the scene is not a grouped clip scene for a group term to act in."""
    if scenario.spawn_law != 'clip_groups':
        raise ValueError("MLAPM: a group term (Ag) was given, but the scene has no groups (scenarios.clip_scenario(groups=))")


def sweep_groups(params):
    """The (Ag, group_dist) pair of every candidate dict, or None when no candidate has a group term.  ValueError when only
    some have one, or on a value group_args refuses."""
    params = list(params)
    have = [isinstance(a, dict) and 'Ag' in a for a in params]
    if any(have) and not all(have):
        raise ValueError(f'simulate_sweep: candidates {[c for c, h in enumerate(have) if not h]} have no group term (Ag) '
                         'and the others do: every candidate or none')
    rows = [group_args({k: a[k] for k in ('Ag', 'group_dist') if k in a}) for a in params if isinstance(a, dict)]
    return rows if any(have) else None


def wall_args(args):
    """(Aw, Bw, wall_cutoff) of MLAPM(**args)'s wall term, None without one.  ValueError: Bw or wall_cutoff without Aw, Aw
    without Bw, a value that is not finite, Aw < 0, Bw > 0, wall_cutoff <= 0."""
    import math
    if 'Aw' not in args:
        if 'Bw' in args or 'wall_cutoff' in args:
            raise ValueError('MLAPM: Bw / wall_cutoff belong to the wall term and need Aw')
        return None
    if 'Bw' not in args:
        raise ValueError('MLAPM: the wall term needs both Aw and Bw')
    Aw, Bw, cutoff = float(args['Aw']), float(args['Bw']), float(args.get('wall_cutoff', DEFAULT_WALL_CUTOFF))
    if not all(math.isfinite(x) for x in (Aw, Bw, cutoff)) or Aw < 0 or Bw > 0 or not cutoff > 0:
        raise ValueError(f'MLAPM: finite Aw >= 0, Bw <= 0 and wall_cutoff > 0 expected, got {Aw}, {Bw}, {cutoff}')
    return Aw, Bw, cutoff


def check_scene_walls(scenario):
    """ValueError when the scene has no valid (finite) obstacle point for a wall term to act from."""
    import torch
    obs = scenario.obstacles
    if obs is None or obs.numel() == 0 or not bool(torch.isfinite(obs.reshape(-1, 2)).all(1).any()):
        raise ValueError('MLAPM: a wall term (Aw) was given, but the scene has no obstacles')


def sweep_walls(params):
    """The (Aw, Bw) pair of every candidate dict, or None when no candidate has a wall term.  ValueError when only some
    have one, or on a value wall_args refuses."""
    params = list(params)
    have = [isinstance(a, dict) and 'Aw' in a for a in params]
    if any(have) and not all(have):
        raise ValueError(f'simulate_sweep: candidates {[c for c, h in enumerate(have) if not h]} have no wall term (Aw, Bw) '
                         'and the others do: every candidate or none')
    for c, a in enumerate(params):
        if isinstance(a, dict) and not have[c] and 'Bw' in a:
            raise ValueError(f'candidate {c}: Bw without Aw')
    if not any(have):
        return None
    return [wall_args({k: a[k] for k in ('Aw', 'Bw') if k in a})[:2] for a in params]


def sweep_laws(params, radius=0.3):
    """The mlapm_law of every candidate dict (simulate_sweep's form).  ValueError on an empty list, an unknown or
    missing key, a value mlapm_law refuses, or candidates with and without a wall term (sweep_walls gives its rows)."""
    from .. import ops_scenario
    params = list(params)
    if not params:
        raise ValueError('simulate_sweep: at least one candidate expected')
    laws = []
    for c, a in enumerate(params):
        if not isinstance(a, dict):
            raise ValueError(f'candidate {c}: a dict in MLAPM(**params) form expected, got {type(a).__name__}')
        unknown = sorted(set(a) - set(SWEEP_KEYS) - set(GROUP_KEYS) - set(NOISE_KEYS))
        missing = [k for k in ('version', 'tau', 'A', 'B') if k not in a]
        if unknown or missing:
            raise ValueError(f'candidate {c}: unknown keys {unknown}, missing keys {missing} (of {SWEEP_KEYS + GROUP_KEYS + NOISE_KEYS})')
        laws.append(ops_scenario.mlapm_law(a['version'], a['tau'], a['A'], a['B'], a.get('C', 0.0), a.get('D', 0.0),
                                           a.get('theta', 0.0), a.get('radius', radius)))
    sweep_walls(params)
    sweep_groups(params)
    sweep_noise(params)
    return laws


class SweepRun:
    """The state, law table (and wall table, when the candidates carry Aw, Bw; and group table, when they carry Ag) and
    captured frames of a sweep of
    n_candidates laws x seeds, kept for running again:
    run(params) writes the candidates' tables into the same device buffers, puts the state back to empty and replays the
    graph captured by the first run, so a further population costs one small copy, the fills and the replays -- what a
    generation of calibrate.calibrate_mlapm_to_stats is.  Every run is bitwise a fresh MLAPM.simulate_sweep."""

    def __init__(self, scenario, frames, n_candidates, seeds, capacity=None, use_graph=None, device='cuda', hist_width=2,
                 frames_per_graph=8, wall_cutoff=DEFAULT_WALL_CUTOFF, nav=None, nav_density=None, exit_choice=None):
        from .. import ops_scenario, scenarios
        self.nav = None if nav is False else nav              # True, or the scene's ops_scenario.nav_field: every run's
        self.nav_density = nav_density                        # None, or the one ops_scenario.nav_density_law of every run
        check_nav_density(self.nav, nav_density)
        self.exit_choice = ops_scenario.resolve_exit_choice(scenario, exit_choice, self.nav)   # None, or every run's law
        if self.nav is not None:
            ops_scenario.nav_wants_sight(self.nav)
            ops_scenario.check_nav_scene(scenario)
        self.seeds = [int(x) for x in seeds]
        self.n_candidates = int(n_candidates)
        if not self.seeds or self.n_candidates < 1:
            raise ValueError('simulate_sweep: at least one candidate and one seed expected')
        if self.n_candidates * len(self.seeds) > ops_scenario.MAX_MEMBERS:
            raise ValueError(f'simulate_sweep: {self.n_candidates} candidates x {len(self.seeds)} seeds = '
                             f'{self.n_candidates * len(self.seeds)} members, more than {ops_scenario.MAX_MEMBERS}')
        self.scenario, self.frames, self.capacity, self.device = scenario, frames, capacity, device
        self.hist_width, self.use_graph, self.frames_per_graph = hist_width, use_graph, frames_per_graph
        self.wall_cutoff = float(wall_cutoff)
        self.st = self.table = self.graph = self.wall_grid = self.wall_table = self.group_table = self.noise_table = None

    def run(self, params, radius=0.3):
        from .. import ops_scenario, scenarios
        params = [dict(a) for a in params]
        laws = sweep_laws(params, radius)
        if len(laws) != self.n_candidates:
            raise ValueError(f'{len(laws)} candidates for a sweep of {self.n_candidates}')
        S = len(self.seeds)
        rows = [law for law in laws for _ in range(S)]
        walls = sweep_walls(params)
        wall_rows = None if walls is None else [ops_scenario.wall_law(*w) for w in walls for _ in range(S)]
        groups = sweep_groups(params)
        group_rows = None if groups is None else [ops_scenario.group_law(*g) for g in groups for _ in range(S)]
        noise = sweep_noise(params)
        dt = float(self.scenario.time_unit)
        noise_rows = None if noise is None else [ops_scenario.noise_law(*z, dt) for z in noise for _ in range(S)]
        if self.st is None:
            if groups is not None:
                check_scene_groups(self.scenario)
            if walls is not None:
                wall_args({'Aw': 0.0, 'Bw': 0.0, 'wall_cutoff': self.wall_cutoff})
                check_scene_walls(self.scenario)
            self.st = scenarios.scenario_state_for(self.scenario, self.frames, self.capacity, self.device, self.hist_width,
                                                   seeds=self.seeds * self.n_candidates)
            self.table = ops_scenario.mlapm_law_table(rows, self.st.p.device)
            if walls is not None:
                self.wall_grid = ops_scenario.wall_grid(self.st.scenario.obstacles, self.wall_cutoff, self.st.p.device)
                self.wall_table = ops_scenario.wall_law_table(wall_rows, self.st.p.device)
            if groups is not None:
                self.group_table = ops_scenario.group_law_table(group_rows, self.st.p.device)
            if noise is not None:
                self.noise_table = ops_scenario.noise_law_table(noise_rows, dt, self.st.p.device)
            if not isinstance(self.nav, ops_scenario.NavField) and self.nav is not None:
                self.nav = ops_scenario.nav_field(self.st.scenario, device=self.st.p.device,
                                                  sight=ops_scenario.nav_wants_sight(self.nav))
            if self.nav_density is not None:
                self.nav_density.radius_cells(self.nav.cell)
                self.nav = ops_scenario.NavFieldDynamic(self.nav, self.st.seeds.numel(), flow=self.nav_density.flow > 0)
        else:
            if (walls is None) != (self.wall_table is None):  # the captured frames are those of the first run's kernel
                raise ValueError('SweepRun: every run of a sweep has a wall term (Aw, Bw) or none has')
            if (groups is None) != (self.group_table is None):
                raise ValueError('SweepRun: every run of a sweep has a group term (Ag) or none has')
            if noise is not None and self.noise_table is None:
                raise ValueError('SweepRun: the first run of this sweep had no fluctuation term (An); its captured frames have none')
            if self.noise_table is not None:                  # (no An in this run: rows of amp 0, which the frame skips)
                ops_scenario.noise_law_table(noise_rows or [(0.0, 0.0)] * len(rows), dt, out=self.noise_table)
            ops_scenario.mlapm_law_table(rows, out=self.table)
            if groups is not None:
                ops_scenario.group_law_table(group_rows, out=self.group_table)
            if walls is not None:
                ops_scenario.wall_law_table(wall_rows, out=self.wall_table)
            ops_scenario.scenario_state_reset(self.st)
        self.graph = MLAPM._run_scenario(self.st, self.table, self.use_graph, self.frames_per_graph, graph=self.graph,
                                         walls=None if walls is None else (self.wall_grid, self.wall_table),
                                         groups=self.group_table, noise=self.noise_table, nav=self.nav,
                                         nav_density=self.nav_density, exit_choice=self.exit_choice)
        ens = scenarios.scenario_result(self.st)
        fields = dict(vars(ens))
        return scenarios.ScenarioSweep(params=params, n_candidates=self.n_candidates, seeds_per_candidate=S, **fields)
