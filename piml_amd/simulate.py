"""Open-world crowd simulation with a trained PINNSF or the closed-form MLAPM law: generate a scene (default: the Grand
Central hall; --scenario crosswalk, four_directional_square, basic_unit1..3 for the reference's synthetic scenes;
--scene-from CLIP.npy for a recorded clip's geometry, first frame and resampled arrivals), simulate it on the GPU and save the result as a v2.2 clip that `RawData.load_trajectory_data` (and so `--iter_flag` pre-training)
reads.

    python -m piml_amd.simulate --checkpoint model.pt --frames 750 --out clip.npy [model flags of piml_amd.main]
    python -m piml_amd.simulate --seeds 0:32 --out 'gc_{seed}.npy'      (an ensemble: every seed in one launch per frame)
    python -m piml_amd.simulate --law mlapm --params params.json --out clip.npy     (MLAPM; params: `calibrate --out`)
    python -m piml_amd.simulate --seeds 0:32 --stats stats.json      (crowd statistics of the run, no clips written)
    python -m piml_amd.simulate --seeds 0:32 --pair-stats pairs.json      (time-to-collision statistics, no clips written)
    python -m piml_amd.simulate --law mlapm --scene-from ucy.npy --seeds 0:32 --pair-stats sim.json   (a clip as the scene)
    python -m piml_amd.simulate --law mlapm --scene-from gc.npy --scene-groups auto --params p.json --seeds 0:32 --group-stats g.json
                                (the clip's groups arrive together; p.json with Ag [, group_dist] adds the group term)
    python -m piml_amd.simulate --law mlapm --scenario gc --params noisy.json --seeds 0:32 --track-stats tracks.json
                                (noisy.json with An [, noise_tau] adds the fluctuation term, in any scene)
    python -m piml_amd.simulate --scenario crosswalk --seeds 0:32 --flow-stats flow.json [--flow-axis x|y|auto|deg]
    python -m piml_amd.simulate --law mlapm --scenario crosswalk --seeds 0:32 --track-stats tracks.json   (track statistics)
                                (velocity correlation and lane order, no clips written)
    python -m piml_amd.simulate --law mlapm --scenario gc --seeds 0:32 --obstacle-stats walls.json   (obstacle statistics)
    python -m piml_amd.simulate --law mlapm --params p.json --seeds 0:32 --obstacle-stats walls.json
                                (p.json with Aw, Bw [, wall_cutoff]: the law with a wall term, e.g. Aw = 50, Bw = -5)
    python -m piml_amd.simulate --law mlapm --scenario gc --seeds 0:32 --line-stats gates.json --lines '0,2,30,2;2,5,2,17'
    python -m piml_amd.simulate --law mlapm --scenario gc --seeds 0:32 --group-stats groups.json        (group statistics)
    python -m piml_amd.simulate --law mlapm --params-sweep a.json b.json --seeds 0:8 --stats sweep.json
                                (one law per file, every law on every seed in ONE ensemble run; statistics per candidate)
    python -m piml_amd.simulate --law mlapm --scene-plan plan.json --nav --seeds 0:32 --obstacle-stats walls.json
                                (a floor plan -- walls as polylines, gates as segments -- routed by a static floor field)
    python -m piml_amd.simulate --law mlapm --scenario gc --nav [--nav-cell 0.25] [--nav-clearance 0.3] --out clip.npy
    python -m piml_amd.simulate --law mlapm --scene-plan plan.json --nav --nav-sight --out clip.npy
                                (the same, steering along lines of sight: the field's any-angle table)
    python -m piml_amd.simulate --law mlapm --scene-plan plan.json --nav --nav-density 2 [--nav-rho0 0.5]
                                [--nav-density-radius 0.75] [--nav-fmax 8] [--nav-every 8]
                                [--nav-solver batch|active [--nav-max-launches N]] --seeds 0:32 --line-stats lines.json
    python -m piml_amd.simulate --law mlapm --scene-plan plan.json --nav --exit-choice [--exit-classes '1,2;3,4']
                                [--exit-margin 1] [--exit-commit 2] [--exit-every 8] --seeds 0:32
                                (the floor field's cost grows with the local density and is solved again every 8 frames)
    python -m piml_amd.simulate --checkpoint model.pt --scene-plan plan.json --route field --seeds 0:32 --obstacle-stats walls.json
                                (the network on a floor plan: --route field|sight steers either law by the floor field)

Model flags (--model, --hidden sizes, --topk_*, --num_history_velocity, ...) are those of `piml_amd.main`, with its
defaults.  Without --checkpoint the network keeps its initial weights (a smoke run)."""
import argparse
import os
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')      # before torch brings the HIP runtime up (piml_amd.hip_graphs_safe)

import torch  # noqa: E402

from . import main as MAIN  # noqa: E402
from . import scenarios as SCENARIOS  # noqa: E402
from .functions import metrics as METRIC  # noqa: E402


def get_args(argv=None):
    p = argparse.ArgumentParser(description='open-world crowd simulation with a trained PINNSF or the MLAPM law')
    p.add_argument('--law', type=str, default='pinnsf', choices=['pinnsf', 'mlapm'],
                   help='force model: the network (default) or the closed-form MLAPM law')
    p.add_argument('--checkpoint', type=str, default='', help='state_dict of the model (torch.save); "" = initial weights')
    p.add_argument('--params', type=str, default=None,
                   help="--law mlapm: the JSON `calibrate --out` writes (version and the six constants, optionally the wall "
                        "term's Aw, Bw, wall_cutoff); default main_mlapm.py's constants, version GC, no wall term")
    p.add_argument('--params-sweep', dest='params_sweep', type=str, nargs='+', default=None,
                   help='--law mlapm with --seeds: several --params files, every law on every seed in one ensemble run '
                        "(MLAPM.simulate_sweep); --stats / --pair-stats / --flow-stats / --track-stats / --obstacle-stats / --line-stats / --group-stats then hold one entry per candidate, pooled over its "
                        "seeds, and --out must contain '{candidate}' and '{seed}'")
    p.add_argument('--mlapm_radius', type=float, default=0.3,
                   help="--law mlapm: MLAPM's UCY collision radius (not the scene's arrival radius)")
    p.add_argument('--scenario', type=str, default='gc', choices=sorted(SCENARIOS.SCENARIOS))
    p.add_argument('--scene-from', dest='scene_from', type=str, default=None,
                   help='build the scene from this recorded v2.2 clip instead of --scenario (scenarios.clip_scenario): its '
                        'obstacles, the agents of its first frame, arrivals resampled from its own tracks at its own rate')
    p.add_argument('--scene-frames', dest='scene_frames', type=str, default=None,
                   help="--scene-from: the window 'a:b' of the clip's frames (default: all)")
    p.add_argument('--scene-jitter', dest='scene_jitter', type=float, default=0.0,
                   help='--scene-from: arrivals start within +- this many metres of the recorded origin (default 0)')
    p.add_argument('--scene-groups', dest='scene_groups', type=str, default=None,
                   help="--scene-from with --law mlapm: keep the clip's groups as arrival units whose members appear "
                        "together (scenarios.clip_scenario(groups=)): 'auto' (the clip's own group statistics) or a JSON "
                        'file holding a list of lists of track indices')
    p.add_argument('--scene-plan', dest='scene_plan', type=str, default=None,
                   help='a floor plan as the scene (scenarios.load_floorplan: JSON with "walls", polylines, and "gates", '
                        'segments); under the network law it needs --route; not with --scenario or --scene-from')
    p.add_argument('--route', type=str, default=None, choices=['field', 'sight'],
                   help='either law with --scenario gc (its route_max_iters becomes 0) or --scene-plan: route the agents by a '
                        "static floor field (ops_scenario.nav_field): 'field' down its gradient, 'sight' along lines of sight "
                        '(the any-angle table as well).  The network is steered by the point one metre down the field in the '
                        "place of its destination; under --law mlapm 'field' is --nav and 'sight' is --nav --nav-sight")
    p.add_argument('--nav', action='store_true',
                   help='--law mlapm with --scenario gc (its route_max_iters becomes 0) or --scene-plan: the agents descend a '
                        'static floor field to their gate instead of walking the straight line (ops_scenario.nav_field)')
    p.add_argument('--nav-cell', dest='nav_cell', type=float, default=None, help='--nav / --route: the grid cell in metres (default 0.25)')
    p.add_argument('--nav-clearance', dest='nav_clearance', type=float, default=None,
                   help='--nav / --route: a cell is blocked when an obstacle point lies within this many metres of its centre '
                        '(default 0.3)')
    p.add_argument('--nav-sight', dest='nav_sight', action='store_true',
                   help='--nav: also build the any-angle table (ops_scenario.nav_field(sight=True)); the agents steer along '
                        'lines of sight, at the next turning point of their shortest path, instead of down the gradient')
    p.add_argument('--nav-density', dest='nav_density', type=float, default=None, metavar='KD',
                   help='--law mlapm --nav: the density-aware floor field (ops_scenario.nav_density_law): a cell\'s travel cost '
                        'is min(1 + KD max(rho - rho0, 0), fmax), and the field is solved again, per member, every --nav-every '
                        'frames, so routed agents go round a congested door; not with --nav-sight, --route sight or --checkpoint')
    p.add_argument('--nav-rho0', dest='nav_rho0', type=float, default=None, help='--nav-density: the density (1/m^2) the cost rises from (default 0.5)')
    p.add_argument('--nav-density-radius', dest='nav_density_radius', type=float, default=None,
                   help='--nav-density: half the side of the square window the density is counted in, metres (default 0.75; '
                        'at most 8 cells)')
    p.add_argument('--nav-fmax', dest='nav_fmax', type=float, default=None, help='--nav-density: the cap of the cost factor (default 8)')
    p.add_argument('--nav-every', dest='nav_every', type=int, default=None,
                   help='--nav-density: frames between two updates of the field (default 8; a multiple of 8, the frames of a '
                        'captured graph, or with --nav-solver active also 1, 2 or 4)')
    p.add_argument('--nav-flow', dest='nav_flow', type=float, default=None, metavar='BETA',
                   help='--nav-density: the direction-aware density: a counted person weighs 1 - BETA (v . d) / vref, d the way '
                        'to the walker\'s gate, so a stream walking the walker\'s way does not close a door and one coming at '
                        'the walker closes it more (default 0: heads are counted)')
    p.add_argument('--nav-vref', dest='nav_vref', type=float, default=None,
                   help='--nav-density --nav-flow: the speed (m/s) at which a person walking the walker\'s way weighs nothing '
                        '(default 1.3)')
    p.add_argument('--nav-solver', dest='nav_solver', choices=('batch', 'active'), default=None,
                   help='--nav-density: how an update is solved: batch (default), batches of 16 dense launches with a host '
                        'read after each; active, one queue of launches that step only the tiles that can still move '
                        '(piml_nav_relax_active): the same field bit for bit, no host read, and --nav-every may also divide 8')
    p.add_argument('--nav-max-launches', dest='nav_max_launches', type=int, default=None, metavar='N',
                   help='--nav-solver active: the launches of an update, an even number >= 2 (default: twice the static '
                        'solve\'s; the run fails at its end when they were too few)')
    p.add_argument('--exit-choice', dest='exit_choice', action='store_true',
                   help='--nav / --route: routed agents re-decide which gate of a class of equivalent exits they leave through '
                        '(ops_scenario.exit_choice_law; the nearest under the static field, the quickest under --nav-density); '
                        'the classes are the plan\'s "exits" unless --exit-classes is given; the report gains the exits per gate')
    p.add_argument('--exit-classes', dest='exit_classes', type=str, default=None, metavar="'1,2;3,4'",
                   help='--exit-choice: the classes of equivalent exits, gate indices separated by commas, classes by semicolons')
    p.add_argument('--exit-margin', dest='exit_margin', type=float, default=None,
                   help='--exit-choice: switch only when the other gate is better by more than this many metres (default 1)')
    p.add_argument('--exit-commit', dest='exit_commit', type=float, default=None,
                   help='--exit-choice: no switch within this many metres of walking distance of the current gate (default 2)')
    p.add_argument('--exit-every', dest='exit_every', type=int, default=None,
                   help='--exit-choice: frames between two passes (default 8)')
    p.add_argument('--frames', type=int, default=750)
    seed = p.add_mutually_exclusive_group()
    seed.add_argument('--seed', type=int, default=0, help='seed of the spawn schedule')
    seed.add_argument('--seeds', type=str, default=None,
                      help="an ensemble, one simulation per seed: 'a:b' (a .. b-1) or 'a,b,c'; --out must contain {seed}")
    p.add_argument('--capacity', type=int, default=None, help='agent slots (default: from the arrival rate)')
    p.add_argument('--out', type=str, default='clip.npy')
    p.add_argument('--stats', type=str, default=None,
                   help='write the crowd statistics (piml_amd.crowdstats, defaults, no box) of the run or ensemble as JSON '
                        'to this path instead of writing clips')
    p.add_argument('--stats-density', dest='stats_density', choices=('gaussian', 'voronoi'), default='gaussian',
                   help='--stats: the local density of the fundamental diagram (DESIGN 4.16 / 4.20)')
    p.add_argument('--stats-cutoff', dest='stats_cutoff', type=float, default=None,
                   help='--stats-density voronoi: the cut-off radius of a cell (default 1.0)')
    p.add_argument('--pair-stats', dest='pair_stats', type=str, default=None,
                   help='write the time-to-collision and pair-distance statistics (piml_amd.pairstats, defaults, no box) '
                        'of the run or ensemble as JSON to this path instead of writing clips')
    p.add_argument('--flow-stats', dest='flow_stats', type=str, default=None,
                   help='write the collective-motion statistics (piml_amd.flowstats: velocity correlation, lane order; '
                        'defaults, no box) of the run or ensemble as JSON to this path instead of writing clips')
    p.add_argument('--flow-axis', dest='flow_axis', type=str, default='x',
                   help="--flow-stats: the lane axis, x, y, auto (principal axis of the velocities) or an angle in degrees")
    p.add_argument('--view-stats', dest='view_stats', type=str, default=None,
                   help='write the heading-frame pair statistics (piml_amd.viewstats: front/back ratio, passing side, '
                        'headway; defaults, no box) of the run or ensemble as JSON to this path instead of writing clips')
    p.add_argument('--view-lags', dest='view_lags', type=str, default='64,128,192',
                   help='--view-stats: the scrambling lags in frames')
    p.add_argument('--track-stats', dest='track_stats', type=str, default=None,
                   help='write the track statistics (piml_amd.trackstats: heading persistence, MSD, acceleration, path '
                        'shape; defaults, dt = the time unit) of the run or ensemble as JSON to this path instead of writing '
                        'clips')
    p.add_argument('--obstacle-stats', dest='obstacle_stats', type=str, default=None,
                   help='write the obstacle statistics (piml_amd.obstaclestats: wall clearance, contacts, crossings, time '
                        "to wall; defaults, no box, the scene's obstacles) of the run or ensemble as JSON to this path "
                        'instead of writing clips')
    p.add_argument('--line-stats', dest='line_stats', type=str, default=None,
                   help='write the measurement-line statistics (piml_amd.linestats: flow, headway, crossing speed, travel '
                        'time; defaults, dt = the time unit) of the run or ensemble across --lines as JSON to this path '
                        'instead of writing clips')
    p.add_argument('--group-stats', dest='group_stats', type=str, default=None,
                   help='write the group statistics (piml_amd.groupstats: who walks with whom, group size, spacing, '
                        'formation; defaults, dt = the time unit) of the run or ensemble as JSON to this path instead of '
                        'writing clips')
    p.add_argument('--lines', type=str, default=None, help="--line-stats: the measurement lines, 'ax,ay,bx,by;ax,ay,bx,by;...'")
    p.add_argument('--time_unit', type=float, default=0.08)
    p.add_argument('--uniform_desired_speed', action=argparse.BooleanOptionalAction, default=None,
                   help="uniform desired speed (default: the scene's own; GC and the crosswalk no, the others yes)")
    own, rest = p.parse_known_args(argv)
    try:
        from .crowdstats import check_density
        check_density(own.stats_density, own.stats_cutoff)
    except ValueError as ex:
        p.error(f'--stats-density / --stats-cutoff: {ex}')
    try:
        from .flowstats import parse_axis
        own.flow_axis = parse_axis(own.flow_axis)
    except ValueError as ex:
        p.error(f'--flow-axis: {ex}')
    try:
        from .pairstats import parse_lags
        from .viewstats import check_options
        own.view_lags = check_options(lags=parse_lags(own.view_lags))[0]
    except ValueError as ex:
        p.error(f'--view-lags: {ex}')
    if (own.line_stats is None) != (own.lines is None):
        p.error('--line-stats needs --lines, and --lines feeds --line-stats only')
    if own.lines is not None:
        try:
            from .linestats import parse_lines
            own.lines = parse_lines(own.lines)
            if isinstance(own.lines, str):
                raise ValueError("'auto' needs a box: give the lines")
        except ValueError as ex:
            p.error(f'--lines: {ex}')
    if own.seeds is not None:
        try:
            own.seeds = parse_seeds(own.seeds)
        except ValueError as ex:
            p.error(f'--seeds: {ex}')
        if '{seed}' not in own.out and not _stats_path(own):
            p.error("--seeds: --out must contain '{seed}' (one clip per seed)")
    if own.scene_from is not None:
        if own.scenario != p.get_default('scenario'):
            p.error('--scene-from builds the scene from a clip: not with --scenario')
        if own.scene_frames is not None:
            try:
                a, b = (int(x) for x in own.scene_frames.split(':'))
            except ValueError:
                p.error(f"--scene-frames: 'a:b' expected, got {own.scene_frames!r}")
            own.scene_frames = (a, b)
        if own.scene_groups is not None and own.law != 'mlapm':
            p.error('--scene-groups: a grouped scene runs under --law mlapm only (the network-driven frame has no group '
                    'arrivals), not with --law pinnsf')
        if own.scene_groups is not None and own.scene_groups != 'auto':
            try:
                own.scene_groups = load_scene_groups(own.scene_groups)
            except (OSError, ValueError) as ex:
                p.error(f'--scene-groups: {ex}')
    elif own.scene_frames is not None or own.scene_jitter != 0.0 or own.scene_groups is not None:
        p.error('--scene-frames / --scene-jitter / --scene-groups need --scene-from')
    own.plan = None
    if own.scene_plan is not None:
        if own.scene_from is not None or own.scenario != p.get_default('scenario'):
            p.error('--scene-plan builds the scene from a floor plan: not with --scene-from or --scenario')
        if own.law != 'mlapm' and own.route is None:
            p.error('--scene-plan: under --law pinnsf a floor plan needs --route field|sight: without the floor field '
                    '(piml_scenario_step_nav) nothing would route the network\'s agents round the walls')
        try:
            own.plan = SCENARIOS.load_floorplan(own.scene_plan)
        except (OSError, ValueError) as ex:
            p.error(f'--scene-plan: {ex}')
    if own.route is not None and own.nav:
        p.error('--route is the law-agnostic spelling of --nav [--nav-sight]: not both')
    if own.route is not None and own.nav_sight:
        p.error('--nav-sight goes with --nav; with --route say --route sight')
    own.routed, own.route_sight = own.nav or own.route is not None, own.nav_sight or own.route == 'sight'
    if own.routed:
        if own.nav and own.law != 'mlapm':
            p.error('--nav is the MLAPM law\'s spelling; the network is routed by the floor field with --route field|sight')
        if own.scene_from is not None or (own.scene_plan is None and own.scenario != 'gc'):
            p.error('--nav / --route route scenes of gates: --scenario gc or --scene-plan (a clip scene carries recorded '
                    'waypoints and no gates; the synthetic scenes have none either)')
        own.nav_cell = 0.25 if own.nav_cell is None else own.nav_cell
        own.nav_clearance = 0.3 if own.nav_clearance is None else own.nav_clearance
        if not (own.nav_cell > 0 and own.nav_cell < float('inf') and own.nav_clearance > 0 and own.nav_clearance < float('inf')):
            p.error(f'--nav-cell / --nav-clearance: finite values > 0 expected, got {own.nav_cell}, {own.nav_clearance}')
    elif own.nav_cell is not None or own.nav_clearance is not None:
        p.error('--nav-cell / --nav-clearance need --nav or --route')
    elif own.nav_sight:
        p.error('--nav-sight needs --nav (it adds the any-angle table to the floor field)')
    own.density_law = None
    if own.nav_density is not None:
        if own.checkpoint or own.law != 'mlapm':
            p.error('--nav-density is built for --law mlapm only: not with --checkpoint or the network law')
        if own.route_sight:
            p.error('--nav-density: the any-angle table is a uniform-cost construction: not with --nav-sight or --route sight')
        if not own.routed:
            p.error('--nav-density needs --nav (the density term belongs to the floor field)')
        from .ops_scenario import nav_density_law
        try:
            own.density_law = nav_density_law(own.nav_density, 0.5 if own.nav_rho0 is None else own.nav_rho0,
                                              0.75 if own.nav_density_radius is None else own.nav_density_radius,
                                              8.0 if own.nav_fmax is None else own.nav_fmax,
                                              8 if own.nav_every is None else own.nav_every,
                                              0.0 if own.nav_flow is None else own.nav_flow,
                                              1.3 if own.nav_vref is None else own.nav_vref,
                                              'batch' if own.nav_solver is None else own.nav_solver, own.nav_max_launches)
            own.density_law.radius_cells(own.nav_cell)
        except ValueError as ex:
            p.error(f'--nav-density: {ex}')
    elif any(x is not None for x in (own.nav_rho0, own.nav_density_radius, own.nav_fmax, own.nav_every, own.nav_flow,
                                     own.nav_vref, own.nav_solver, own.nav_max_launches)):
        p.error('--nav-rho0 / --nav-density-radius / --nav-fmax / --nav-every / --nav-flow / --nav-vref / --nav-solver / '
                '--nav-max-launches need --nav-density')
    own.exit_law = None
    if own.exit_choice:
        if not own.routed:
            p.error('--exit-choice reads the floor field: it needs --nav or --route field|sight')
        from .ops_scenario import exit_choice_law
        try:
            classes = parse_exit_classes(own.exit_classes) if own.exit_classes is not None else \
                (own.plan.exit_classes if own.plan is not None else None)
            if not classes:
                raise ValueError('no classes: give --exit-classes \'1,2;3,4\' or a plan with "exits"')
            own.exit_law = exit_choice_law(classes, 1.0 if own.exit_margin is None else own.exit_margin,
                                           2.0 if own.exit_commit is None else own.exit_commit,
                                           8 if own.exit_every is None else own.exit_every)
            own.exit_law.gate_class_host(own.plan.entries.shape[0] if own.plan is not None else 7)    # (GC has 7 gates)
        except ValueError as ex:
            p.error(f'--exit-choice: {ex}')
    elif any(x is not None for x in (own.exit_classes, own.exit_margin, own.exit_commit, own.exit_every)):
        p.error('--exit-classes / --exit-margin / --exit-commit / --exit-every need --exit-choice')
    if own.params_sweep is not None:
        if own.params is not None:
            p.error('--params-sweep takes the place of --params: not both')
        if own.law != 'mlapm' or own.seeds is None:
            p.error('--params-sweep needs --law mlapm and --seeds')
        if not _stats_path(own) and '{candidate}' not in own.out:
            p.error("--params-sweep: --out must contain '{candidate}' and '{seed}' (one clip per candidate and seed)")
    if own.law == 'mlapm':
        if own.checkpoint:
            p.error('--checkpoint is a PINNSF state_dict: not with --law mlapm (use --params)')
        try:
            own.mlapm = load_mlapm_params(own.params)
            own.mlapm_sweep = None if own.params_sweep is None else [load_mlapm_params(f) for f in own.params_sweep]
            if own.mlapm_sweep is not None:
                own.mlapm_sweep, own.wall_cutoff = _sweep_candidates(own.mlapm_sweep)
        except (OSError, ValueError) as ex:
            p.error(f'--params / --params-sweep: {ex}')
    elif own.params is not None:
        p.error('--params needs --law mlapm')
    model_args = MAIN.get_args(rest)
    return own, model_args


def parse_exit_classes(text):
    """--exit-classes '1,2;3,4' -> [[1, 2], [3, 4]].  ValueError on anything else."""
    try:
        return [[int(g) for g in c.split(',')] for c in text.split(';')]
    except ValueError:
        raise ValueError(f"--exit-classes: gate indices separated by ',' and classes by ';' expected, got {text!r}") from None


def load_scene_groups(path):
    """--scene-groups FILE.json: a list of lists of track indices.  ValueError on anything else."""
    import json
    with open(path) as fh:
        got = json.load(fh)
    if not isinstance(got, list) or not all(isinstance(g, list) and all(isinstance(i, int) and not isinstance(i, bool)
                                                                         for i in g) for g in got):
        raise ValueError(f'{path}: a JSON list of lists of track indices expected')
    return got


def load_mlapm_params(path):
    """MLAPM's constructor arguments from the JSON `python -m piml_amd.calibrate --out` writes ({'version', 'tau', 'A',
    'B', 'C', 'D', 'theta'} and, for a law with a wall term, 'Aw', 'Bw', 'wall_cutoff'; for one with a group term, 'Ag' and
    optionally 'group_dist'; for one with a fluctuation term, 'An' and optionally 'noise_tau'); constants the file leaves out keep
    calibrate.DEFAULT_INIT's values (main_mlapm.py:16) -- the wall term has no default: without Aw there is none --, and
    path None is those constants with version GC.  ValueError on an unknown version, an unknown key, a non-number or a
    wall term MLAPM refuses (Bw or wall_cutoff without Aw, Aw < 0, Bw > 0, wall_cutoff <= 0) or a group term it refuses
    (group_dist without Ag, a negative value) or a fluctuation term it refuses (noise_tau without An, a negative value)."""
    import json
    from . import calibrate, ops
    params = {'version': 'GC', **calibrate.DEFAULT_INIT}
    if path is None:
        return params
    with open(path) as fh:
        got = json.load(fh)
    if not isinstance(got, dict):
        raise ValueError(f'{path}: a JSON object expected')
    numbers = calibrate.PARAM_NAMES + calibrate.WALL_PARAM_NAMES + ('wall_cutoff', 'Ag', 'group_dist', 'An', 'noise_tau')
    unknown = sorted(set(got) - {'version', *numbers})
    if unknown:
        raise ValueError(f'{path}: unknown keys {unknown} (expected version and {list(numbers)})')
    if got.get('version', 'GC') not in ops.MLAPM_VARIANTS:
        raise ValueError(f"{path}: unknown version {got.get('version')!r} (one of {sorted(ops.MLAPM_VARIANTS)})")
    for k in numbers:
        if k in got and (isinstance(got[k], bool) or not isinstance(got[k], (int, float))):
            raise ValueError(f'{path}: {k} = {got[k]!r} is not a number')
    params.update(got)
    from .models.mlapm import group_args, noise_args, wall_args
    try:
        wall_args(params)
        group_args(params)
        noise_args(params)
    except ValueError as ex:
        raise ValueError(f'{path}: {ex}') from None
    return params


def _sweep_candidates(params):
    """--params-sweep: the candidates without their wall_cutoff, and the one cutoff they share (a sweep runs on one wall
    grid).  ValueError when the files disagree on it or only some carry a wall term."""
    from .models.mlapm import DEFAULT_WALL_CUTOFF, sweep_walls
    sweep_walls(params)
    cut = sorted({float(a.get('wall_cutoff', DEFAULT_WALL_CUTOFF)) for a in params if 'Aw' in a})
    if len(cut) > 1:
        raise ValueError(f'the files disagree on wall_cutoff ({cut}): a sweep runs on one wall grid')
    return [{k: v for k, v in a.items() if k != 'wall_cutoff'} for a in params], (cut[0] if cut else DEFAULT_WALL_CUTOFF)


def parse_seeds(text):
    """'a:b' -> [a, ..., b-1]; 'a,b,c' -> [a, b, c].  ValueError on anything else or on no seed at all."""
    text = text.strip()
    if ':' in text:
        lo, hi = (int(x) for x in text.split(':'))
        seeds = list(range(lo, hi))
    else:
        seeds = [int(x) for x in text.split(',')]
    if not seeds:
        raise ValueError(f'no seed in {text!r}')
    return seeds


def _report(tag, frames, res, threshold, out, soft=None, hard=None):
    """(spawned, retired, dropped, soft, hard) of one simulation and its line, as piml_amd.main reports collisions."""
    n = res.num_agents
    retired = n - int(res.mask_p[-1, :n].sum().item())
    if soft is None:
        pos = res.position[:, :n]
        soft = METRIC.collision_count(pos, threshold, reduction='sum')
        hard = METRIC.collision_count(pos, threshold / 2, reduction='sum')
    print(f'[simulate] {tag}: {frames} frames, capacity {res.capacity}: spawned {res.spawned}, '
          f'retired {retired}, dropped {res.dropped}; collisions soft {soft:g} hard {hard:g}; saved {out}')
    if getattr(res, 'exit_switches', None) is not None:      # a run with an exit choice: who left where
        print(f'[simulate] {tag}: exits per gate {res.exit_counts()}, switches {int(res.exit_switches[:n].sum().item())}')
    return res.spawned, retired, res.dropped, soft, hard


def main(argv=None):
    own, args = get_args(argv)
    MAIN.set_exp_configs(args)
    if own.law == 'mlapm':
        from .models.mlapm import MLAPM
        sim = MLAPM(**own.mlapm)
        run_kw = dict(radius=own.mlapm_radius, device=args.device, hist_width=2 * args.num_history_velocity)
    else:
        from .models.simulators import BaseSimulator
        # the feature widths piml_amd.data.dataset sets from a clip: 6-wide neighbour rows, self = (dest, history, a, v0)
        args.ped_feature_dim = args.obs_feature_dim = 6
        args.self_feature_dim = 5 + 2 * args.num_history_velocity
        sim = BaseSimulator(args)
        if own.checkpoint:
            sim.model.load_state_dict(torch.load(own.checkpoint, map_location=args.device))
        sim.model.eval()
        run_kw = {}
    if own.scene_from is not None:
        scenario = _clip_scene(own)
        own.scenario = scenario.name
    elif own.plan is not None:
        scenario = own.plan
        own.scenario = scenario.name
    else:
        kw = {} if own.uniform_desired_speed is None else {'uniform_desired_speed': own.uniform_desired_speed}
        scenario = SCENARIOS.SCENARIOS[own.scenario](time_unit=own.time_unit, **kw)
    if own.law == 'mlapm' and any('Aw' in a for a in (own.mlapm_sweep or [own.mlapm])):
        from .models.mlapm import check_scene_walls
        try:
            check_scene_walls(scenario)
        except ValueError as ex:
            sys.exit(f'--params / --params-sweep: {ex}')
    if own.law == 'mlapm' and any('Ag' in a for a in (own.mlapm_sweep or [own.mlapm])):
        from .models.mlapm import check_scene_groups
        try:
            check_scene_groups(scenario)
        except ValueError as ex:
            sys.exit(f'--params / --params-sweep: {ex} (--scene-from CLIP --scene-groups auto|FILE.json)')
    if own.routed:
        import dataclasses
        from . import ops_scenario
        scenario = dataclasses.replace(scenario, route_max_iters=0)       # (GC: the field routes, not the pillar's detour)
        try:
            run_kw['nav'] = ops_scenario.nav_field(scenario.to(args.device), cell=own.nav_cell, clearance=own.nav_clearance,
                                                   device=args.device, sight=own.route_sight)
        except (ValueError, RuntimeError) as ex:
            sys.exit(f'--nav / --route: {ex}')
        print(f'[simulate] floor field: {run_kw["nav"].G} gates, {run_kw["nav"].gx} x {run_kw["nav"].gy} cells of '
              f'{run_kw["nav"].cell:g} m, {run_kw["nav"].iterations} steps')
        if own.route_sight:
            print(f'[simulate] lines of sight: {run_kw["nav"].sight_iterations} steps')
        if own.density_law is not None:
            run_kw['nav_density'] = own.density_law
            print(f'[simulate] density term: {own.density_law}')
        if own.exit_law is not None:
            run_kw['exit_choice'] = own.exit_law
            print(f'[simulate] exit choice: {own.exit_law}')
    if own.law == 'mlapm' and own.mlapm_sweep is not None:
        return _sweep(sim, scenario, own, run_kw)
    if own.seeds is not None:
        return _ensemble(sim, scenario, own, args, run_kw)
    res = sim.simulate_scenario(scenario, own.frames, seed=own.seed, capacity=own.capacity, **run_kw)
    if _stats_path(own):
        _stats(res, own)
    else:
        res.save_data(own.out)
    _report(own.scenario, own.frames, res, args.collision_threshold, _stats_path(own) or own.out)
    return res


def _clip_scene(own):
    """--scene-from: scenarios.clip_scenario of the clip (its own time unit and desired speeds; --time_unit and
    --uniform_desired_speed do not apply)."""
    from .data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(own.scene_from)
    try:
        return SCENARIOS.clip_scenario(raw, frames=own.scene_frames, jitter=own.scene_jitter, groups=getattr(own, 'scene_groups', None))
    except ValueError as ex:
        sys.exit(f'--scene-from {own.scene_from}: {ex}')


def _stats_path(own):
    return ', '.join(p for p in (own.stats, own.pair_stats, own.flow_stats, own.track_stats, own.obstacle_stats, own.line_stats,
                                 own.group_stats, own.view_stats)
                     if p is not None)


def _crowd_kw(own):
    return {} if own.stats_density == 'gaussian' else dict(density=own.stats_density, cutoff=own.stats_cutoff)


def _stats(res, own):
    """--stats / --pair-stats / --flow-stats / --track-stats / --obstacle-stats / --line-stats / --group-stats: the CrowdStats /
    PairStats / FlowStats / TrackStats / ObstacleStats / LineStats / GroupStats JSON of a run or an ensemble (one call for every member)."""
    if own.stats is not None:
        from . import crowdstats
        st = res.crowd_stats(**_crowd_kw(own))
        st.to_json(own.stats)
        crowdstats.print_diagram(st, 'simulate --stats')
    if own.pair_stats is not None:
        from . import pairstats
        ps = res.pair_stats()
        ps.to_json(own.pair_stats)
        pairstats.print_pair_stats(ps, 'simulate --pair-stats')
    if own.flow_stats is not None:
        from . import flowstats
        fs = res.flow_stats(axis=own.flow_axis)
        fs.to_json(own.flow_stats)
        flowstats.print_flow_stats(fs, 'simulate --flow-stats')
    if own.track_stats is not None:
        from . import trackstats
        ts = res.track_stats()
        ts.to_json(own.track_stats)
        trackstats.print_track_stats(ts, 'simulate --track-stats')
    if own.obstacle_stats is not None:
        from . import obstaclestats
        try:
            os_ = res.obstacle_stats()
        except ValueError as ex:
            sys.exit(f'--obstacle-stats: {ex}')
        os_.to_json(own.obstacle_stats)
        obstaclestats.print_obstacle_stats(os_, 'simulate --obstacle-stats')
    if own.line_stats is not None:
        from . import linestats
        ls = res.line_stats(own.lines)
        ls.to_json(own.line_stats)
        linestats.print_line_stats(ls, 'simulate --line-stats')
    if own.group_stats is not None:
        from . import groupstats
        gs = res.group_stats()
        gs.to_json(own.group_stats)
        groupstats.print_group_stats(gs, 'simulate --group-stats')
    if own.view_stats is not None:
        from . import viewstats
        vs = res.view_stats(lags=own.view_lags)
        vs.to_json(own.view_stats)
        viewstats.print_view_stats(vs, 'simulate --view-stats')
    if getattr(own, 'exit_law', None) is not None:
        _add_exit_counts(res, own)


def _add_exit_counts(res, own):
    """--exit-choice: every statistics JSON of the run gains 'exit_counts' (retired agents per gate; per member for an
    ensemble) and 'exit_switches' (the switches made), beside what the statistics wrote (their readers ignore other keys)."""
    import json
    counts, switches = res.exit_counts(), int(res.exit_switches.sum().item())
    for path in (own.stats, own.pair_stats, own.flow_stats, own.track_stats, own.obstacle_stats, own.line_stats, own.group_stats,
                 own.view_stats):
        if path is None:
            continue
        with open(path) as fh:
            got = json.load(fh)
        if isinstance(got, dict):
            got['exit_counts'], got['exit_switches'] = counts, switches
            with open(path, 'w') as fh:
                json.dump(got, fh)


def _sweep(sim, scenario, own, run_kw):
    """--params-sweep: every law on every seed in one ensemble run; statistics per candidate, pooled over its seeds."""
    import json
    sw = sim.simulate_sweep(scenario, own.frames, own.mlapm_sweep, own.seeds, capacity=own.capacity,
                            wall_cutoff=own.wall_cutoff, **run_kw)
    groups = [sw.members_of(c) for c in range(sw.n_candidates)]
    if own.stats is not None:
        from . import crowdstats
        st = sw.crowd_stats(**_crowd_kw(own))
        crowdstats.print_dropped(st, 'simulate --stats')
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': st.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.pair_stats is not None:
        ps = sw.pair_stats()
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': ps.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.pair_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.flow_stats is not None:
        fs = sw.flow_stats(axis=own.flow_axis)
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': fs.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.flow_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.track_stats is not None:
        ts = sw.track_stats()
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': ts.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.track_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.obstacle_stats is not None:
        try:
            os_ = sw.obstacle_stats()
        except ValueError as ex:
            sys.exit(f'--obstacle-stats: {ex}')
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': os_.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.obstacle_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.line_stats is not None:
        ls = sw.line_stats(own.lines)
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': ls.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.line_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.group_stats is not None:
        gs = sw.group_stats()
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': gs.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.group_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    if own.view_stats is not None:
        vs = sw.view_stats(lags=own.view_lags)
        entries = [{'params': sw.params[c], 'file': own.params_sweep[c], 'stats': vs.select(g).pooled().to_json()}
                   for c, g in enumerate(groups)]
        with open(own.view_stats, 'w') as fh:
            json.dump({'seeds': own.seeds, 'candidates': entries}, fh)
    where = _stats_path(own)
    if not where:
        sw.save_data(own.out)
        where = own.out
    for c, g in enumerate(groups):
        spawned = [sw.spawned[m] for m in g]
        dropped = [sw.dropped[m] for m in g]
        print(f'[simulate] {own.scenario} candidate {c} ({own.params_sweep[c]}): {len(g)} seeds x {own.frames} frames, '
              f'capacity {sw.capacity}: spawned {sum(spawned)}, dropped {sum(dropped)}; saved {where}')
        if getattr(sw, 'exit_switches', None) is not None:
            counts = sw.exit_counts()
            print(f'[simulate] candidate {c}: exits per gate {[sum(counts[m][e] for m in g) for e in range(sw.num_gates)]}')
    return sw


def _ensemble(sim, scenario, own, args, run_kw):
    ens = sim.simulate_ensemble(scenario, own.frames, own.seeds, capacity=own.capacity, **run_kw)
    if _stats_path(own):
        _stats(ens, own)
        paths = [_stats_path(own)] * len(ens)
    else:
        paths = ens.save_data(own.out)
    soft = ens.collision_counts(args.collision_threshold)
    hard = ens.collision_counts(args.collision_threshold / 2)
    rows = [_report(f'{own.scenario} (seed {s})', own.frames, ens.member(m), args.collision_threshold, paths[m], soft[m], hard[m])
            for m, s in enumerate(ens.seeds)]
    stats = torch.tensor(rows, dtype=torch.float64)
    mean, std = stats.mean(0), stats.std(0, unbiased=False)
    print(f'[simulate] {own.scenario}: {len(ens)} seeds, mean +- std: ' + ', '.join(
        f'{k} {mean[j]:.4g} +- {std[j]:.3g}' for j, k in enumerate(('spawned', 'retired', 'dropped', 'soft', 'hard'))))
    return ens


if __name__ == '__main__':
    main(sys.argv[1:])
