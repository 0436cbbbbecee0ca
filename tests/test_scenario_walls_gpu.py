"""GPU: the MLAPM scenario frame with the wall term (piml_scenario_step_mlapm_walls; MLAPM(..., Aw=, Bw=) in
simulate_scenario / simulate_ensemble / simulate_sweep and the statistics fit) on the four-directional square and the Grand
Central hall, 3 seeds x 40 frames: Aw = 0 is the plain run, the first frame's acceleration is the plain one plus the
operator's wall force, members / table forms / captured replays / re-run sweeps are bitwise each other, the arrivals do not
move, the walls push the right way, and a short statistics fit of (Aw, Bw) runs."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_pairstats_gpu import GC_CLIP, _raw
from test_scenario_mlapm_gpu import FIELDS, LAW, _same, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS, FRAMES = [0, 1, 2], 40                    # the window of the obstacle statistics' GPU test
AW, BW, CUTOFF = 50.0, -5.0, 2.0                 # Helbing and Molnar 1995
PLAIN = dict(version='GC', **LAW)
WALLED = dict(PLAIN, Aw=AW, Bw=BW)
# gc: 4094 obstacle points.  square: the reference's scene (128 points, 100 agents), whose agents start 7 m from the
# circle and do not reach it in 40 frames.  small_square: the same scene with 36 agents that start 1 - 1.4 m from it.
SCENES = ('gc', 'square', 'small_square')


@functools.lru_cache(maxsize=None)
def scene(name):
    from piml_amd import scenarios
    if name == 'gc':
        return scenarios.gc_scenario().to(DEV)
    if name == 'square':
        return scenarios.four_directional_square_scenario().to(DEV)
    return scenarios.four_directional_square_scenario(block_length=6.0, peds_density=3).to(DEV)


def MLAPM(**params):
    from piml_amd.models.mlapm import MLAPM as M
    return M(**params)


@functools.lru_cache(maxsize=None)
def ensemble(name, walled):
    """the shared runs: the plain law's ensemble, and the walled law's with the same capacity"""
    if not walled:
        return MLAPM(**PLAIN).simulate_ensemble(scene(name), FRAMES, SEEDS)
    return MLAPM(**WALLED).simulate_ensemble(scene(name), FRAMES, SEEDS, capacity=ensemble(name, False).capacity)


def same_values(a, b, fields=FIELDS):
    """torch.equal of every recorded tensor (NaN positions of absent slots compare as equal)"""
    return all(torch.equal(torch.nan_to_num(getattr(a, k).float(), 1e30), torch.nan_to_num(getattr(b, k).float(), 1e30)) and
               torch.equal(getattr(a, k).isnan(), getattr(b, k).isnan()) for k in fields)


@pytest.mark.parametrize('name', SCENES)
def test_zero_strength_is_the_plain_run(name):
    plain = ensemble(name, False)
    zero = MLAPM(**PLAIN, Aw=0.0, Bw=BW).simulate_ensemble(scene(name), FRAMES, SEEDS, capacity=plain.capacity)
    assert same_values(zero, plain) and zero.spawned == plain.spawned and zero.dropped == plain.dropped
    assert same_values(MLAPM(**PLAIN, Aw=0.0, Bw=0.0, wall_cutoff=0.5).simulate_scenario(scene(name), FRAMES, seed=SEEDS[1],
                                                                                      capacity=plain.capacity),
                       plain.member(1))


@pytest.mark.parametrize('name', SCENES)
def test_first_frame_adds_the_operators_wall_force(name):
    """acceleration[1] == acceleration_plain[1] + wall_force(position[0]) for the present slots, bitwise: the same wave
    function on the same inputs, and one float32 add (the build never contracts)"""
    from piml_amd import ops_scenario
    plain, walled = ensemble(name, False), ensemble(name, True)
    assert torch.equal(bits(walled.position[:, 0]), bits(plain.position[:, 0]))
    grid = ops_scenario.wall_grid(scene(name).obstacles, CUTOFF, DEV)
    W, d2, idx = ops_scenario.wall_force(plain.position[:, 0], grid, AW, BW, return_selection=True)
    present = (plain.mask_p[:, 0] == 1) & (plain.mask_p[:, 1] == 1) & (walled.mask_p[:, 1] == 1)
    want = plain.acceleration[:, 1] + W
    felt = present & (idx >= 0)
    print(f'\n[walls] {name}: {int(present.sum())} present slots in frame 0, {int(felt.sum())} within {CUTOFF} m of a wall, '
          f'largest wall force {float(W[present].norm(dim=-1).max()):.3f} m/s^2')
    assert int(present.sum()) > 0
    assert torch.equal(bits(walled.acceleration[:, 1][present]), bits(want[present]))
    assert (W[present & (idx < 0)] == 0).all()
    if name != 'square':
        assert int(felt.sum()) > 0 and not torch.equal(bits(walled.acceleration[:, 1]), bits(plain.acceleration[:, 1]))
        assert not same_values(walled, plain, ('position',))
    else:                                                         # nobody comes within the cutoff: the plain run
        assert same_values(walled, plain)
    # v' = v + F dt, p' = p + v' dt with the frame's force
    dt = float(plain.time_unit)
    v1 = walled.velocity[:, 0] + walled.acceleration[:, 1] * dt
    assert torch.equal(bits(walled.velocity[:, 1][present]), bits(v1[present]))
    assert torch.equal(bits(walled.position[:, 1][present]), bits((walled.position[:, 0] + v1 * dt)[present]))


def run_state(name, law, walls, capacity, frames=12, use_graph=False):
    from piml_amd import scenarios
    from piml_amd.models.mlapm import MLAPM as M
    st = scenarios.scenario_state_for(scene(name), frames, capacity, DEV, seeds=SEEDS)
    M._run_scenario(st, law, use_graph, 4, walls=walls)
    return scenarios.scenario_result(st)


@pytest.mark.parametrize('name', ['gc', 'small_square'])
def test_members_table_forms_and_captured_replay_are_bitwise_equal(name):
    from piml_amd import hip_graphs_safe, ops_scenario
    assert hip_graphs_safe()
    ens = ensemble(name, True)
    for m, s in enumerate(SEEDS):                                 # member m of an ensemble is the single run
        one = MLAPM(**WALLED).simulate_scenario(scene(name), FRAMES, seed=s, capacity=ens.capacity)
        assert _same(ens.member(m), one), m
    # the four forms of the entry: law by value / table x wall by value / table
    law = ops_scenario.mlapm_law(**{**LAW, 'version': 'GC'})
    wall = ops_scenario.wall_law(AW, BW)
    table = ops_scenario.mlapm_law_table([law] * len(SEEDS), DEV)
    wtable = ops_scenario.wall_law_table([(AW, BW)] * len(SEEDS), DEV)
    grid = ops_scenario.wall_grid(scene(name).obstacles, CUTOFF, DEV)
    base = run_state(name, law, (grid, wall), ens.capacity)
    for k in FIELDS:                                              # ... which is the ensemble's first 12 frames
        x, y = getattr(base, k), getattr(ens, k)
        if x.dim() >= 3 and x.shape[1] == 12 and y.shape[1] == FRAMES:
            assert torch.equal(bits(x), bits(y[:, :12])), k
    for lw, wl in ((law, wtable), (table, wall), (table, wtable)):
        other = run_state(name, lw, (grid, wl), ens.capacity)
        assert all(_same(other.member(m), base.member(m)) for m in range(len(SEEDS)))
    captured = run_state(name, table, (grid, wtable), ens.capacity, use_graph=True)            # 1 eager + 2 replays of 4 + 2
    assert all(_same(captured.member(m), base.member(m)) for m in range(len(SEEDS)))
    graph = MLAPM(**WALLED).simulate_ensemble(scene(name), FRAMES, SEEDS, capacity=ens.capacity, use_graph=True)
    eager = MLAPM(**WALLED).simulate_ensemble(scene(name), FRAMES, SEEDS, capacity=ens.capacity, use_graph=False)
    assert all(_same(graph.member(m), eager.member(m)) and _same(graph.member(m), ens.member(m)) for m in range(len(SEEDS)))
    # a one-candidate sweep (both tables) is the ensemble
    sw = MLAPM(**PLAIN).simulate_sweep(scene(name), FRAMES, [WALLED], SEEDS, capacity=ens.capacity)
    assert all(_same(sw.member(m), ens.member(m)) for m in range(len(SEEDS)))


def _snapshot(sw):
    return {k: getattr(sw, k).clone() for k in FIELDS}, list(sw.spawned), list(sw.dropped)


def test_sweep_run_twice_with_other_wall_rows_equals_fresh_runs():
    from piml_amd.models.mlapm import SweepRun
    name, seeds = 'small_square', SEEDS[:2]
    first = [dict(WALLED), dict(WALLED, Aw=5.0, Bw=-1.0)]
    second = [dict(WALLED, Aw=120.0, Bw=-8.0, tau=0.6), dict(WALLED, Aw=0.0)]
    run = SweepRun(scene(name), FRAMES, 2, seeds)
    got = []
    for params in (first, second, first):
        got.append(_snapshot(run.run(params)))
    assert run.graph is not None and run.wall_table.shape == (4, 2)
    for params, (fields, spawned, dropped) in zip((first, second, first), got):
        fresh = MLAPM(**PLAIN).simulate_sweep(scene(name), FRAMES, params, seeds, capacity=run.st.capacity)
        for k in FIELDS:
            assert torch.equal(bits(fields[k]), bits(getattr(fresh, k))), k
        assert spawned == fresh.spawned and dropped == fresh.dropped
        for c, p in enumerate(params):                            # and each candidate is its own ensemble
            ens = MLAPM(**p).simulate_ensemble(scene(name), FRAMES, seeds, capacity=run.st.capacity)
            assert all(_same(fresh.member(c * 2 + k), ens.member(k)) for k in range(2)), c
    assert not torch.equal(bits(got[0][0]['position']), bits(got[1][0]['position']))
    with pytest.raises(ValueError):
        run.run([dict(PLAIN), dict(PLAIN)])                       # the captured frames are the wall kernel's
    with pytest.raises(ValueError):
        MLAPM(**PLAIN).simulate_sweep(scene(name), 5, [dict(WALLED), dict(PLAIN)], seeds)


@pytest.mark.parametrize('name', SCENES)
def test_arrivals_do_not_depend_on_the_walls(name):
    """spawns, spawned, dropped, desired_speed and the waypoints are bitwise the plain run's: they depend on seed, frame and
    ordinal only"""
    plain, walled = ensemble(name, False), ensemble(name, True)
    assert walled.spawned == plain.spawned and walled.dropped == plain.dropped and walled.capacity == plain.capacity
    for k in ('spawn_count', 'desired_speed', 'waypoints'):
        assert torch.equal(bits(getattr(walled, k)), bits(getattr(plain, k))), k
    # every agent appears where and when it does in the plain run
    born = torch.zeros_like(plain.mask_p, dtype=torch.bool)
    born[:, 0] = plain.mask_p[:, 0] == 1
    born[:, 1:] = (plain.mask_p[:, 1:] == 1) & (plain.mask_p[:, :-1] == 0)
    assert torch.equal(bits(walled.position[born]), bits(plain.position[born])) and int(born.sum()) >= sum(
        min(n, plain.capacity) for n in plain.spawned)


def test_walls_push_the_right_way_on_gc():
    """direction only: with Aw = 50, Bw = -5 the share of tracks that cross an obstacle and the contact rate are not above
    the plain law's; nothing more is asserted, nobody has measured these"""
    plain, walled = ensemble('gc', False).obstacle_stats(), ensemble('gc', True).obstacle_stats()
    for tag, st in (('plain', plain), (f'Aw={AW:g}, Bw={BW:g}', walled)):
        print(f'\n[walls] GC, seeds {SEEDS} x {FRAMES} frames, {tag}: hit_track_fraction {st.hit_track_fraction():.4f}, '
              f'contact_rate {st.contact_rate():.5f}, contact_track_fraction {st.contact_track_fraction():.4f}, '
              f'hit_rate {st.hit_rate():.5f}, mean clearance {st.mean_clearance():.3f} m')
    assert walled.hit_track_fraction() <= plain.hit_track_fraction()
    assert walled.contact_rate() <= plain.contact_rate()


def test_statistics_fit_of_the_wall_constants():
    from piml_amd import calibrate
    from piml_amd.obstaclestats import obstacle_stats_of_raw
    sc = scene('gc')
    ref = obstacle_stats_of_raw(_raw(GC_CLIP), sc.obstacles, frames=(0, FRAMES))
    res = calibrate.calibrate_mlapm_to_stats(sc, (None, None, ref), init={'Aw': AW, 'Bw': BW}, fit=('Aw', 'Bw'),
                                             frames=FRAMES, seeds=SEEDS[:2], population=4, generations=2)
    print(f'\n[walls] statistics fit, 2 generations x 4 candidates x 2 seeds: objective {res.initial_loss:.4f} -> '
          f'{res.final_loss:.4f}, Aw {res.params["Aw"]:.3f}, Bw {res.params["Bw"]:.3f}, terms {res.terms}')
    assert res.status == 'ok' and res.fit == ('Aw', 'Bw')
    assert math.isfinite(res.params['Aw']) and math.isfinite(res.params['Bw'])
    assert res.params['Aw'] >= 0.0 and res.params['Bw'] <= 0.0 and res.params['wall_cutoff'] == CUTOFF
    assert all(res.params[k] == PLAIN[k] for k in LAW)            # the pair law's constants are carried through
    assert len(res.history) == 2 and res.history[1] <= res.history[0] <= res.initial_loss and math.isfinite(res.history[1])
    assert set(calibrate.OBJECTIVE_KEYS['obstacles']) <= set(res.terms)
    json.dumps(res.params)                                        # what calibrate --out writes


def test_errors_and_the_command_line(tmp_path):
    from piml_amd import ops_scenario, scenarios, simulate
    with pytest.raises(ValueError, match='no obstacles'):
        MLAPM(**WALLED).simulate_scenario(scenarios.crosswalk_scenario().to(DEV), 5)
    sc = scene('small_square')
    st = scenarios.scenario_state_for(sc, 4, 40, DEV, seeds=SEEDS)
    ops_scenario.scenario_step(st, init=True)
    law, grid = ops_scenario.mlapm_law(), ops_scenario.wall_grid(sc.obstacles, CUTOFF, DEV)
    with pytest.raises(ValueError):
        ops_scenario.scenario_step_mlapm(st, law, walls=(grid, ops_scenario.wall_law_table([(AW, BW)] * 2, DEV)))
    with pytest.raises(TypeError):
        ops_scenario.scenario_step_mlapm(st, law, walls=(grid, (AW, BW)))
    assert int(st.t.item()) == 0
    params = tmp_path / 'walled.json'
    params.write_text(json.dumps(dict(WALLED, wall_cutoff=CUTOFF)))
    out = tmp_path / 'walls.json'
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--law', 'mlapm', '--params', str(params), '--scenario',
                        'gc', '--frames', '12', '--seeds', '0:2', '--obstacle-stats', str(out)], cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    from piml_amd.obstaclestats import ADDITIVE, ObstacleStats
    got = ObstacleStats.from_json(str(out))
    want = MLAPM(**WALLED).simulate_ensemble(scene('gc'), 12, [0, 1]).obstacle_stats()
    assert got.options['n_obstacles'] == 4094 and all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ADDITIVE)
    plain = MLAPM(**PLAIN).simulate_ensemble(scene('gc'), 12, [0, 1]).obstacle_stats()
    assert not all(np.array_equal(getattr(plain, k), getattr(want, k)) for k in ADDITIVE)       # the file's wall term ran
