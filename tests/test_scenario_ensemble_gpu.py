"""GPU: ensembles of an open-world scene (piml_scenario_step_members, BaseSimulator.simulate_ensemble): member m bitwise
the single-scene frame of seed seeds[m] in every scene, the simulator end to end against simulate_scenario, the per-member
clips and collision counts, the CLI's --seeds and the operators' argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scenario_ref
import scenario_synth_ref
from conftest import REPO
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCENES = ('gc', 'crosswalk', 'four_directional_square', 'basic_unit1', 'basic_unit2', 'basic_unit3')
SEEDS = [0, 5, (1 << 33) + 7]            # the last one's key has a high word


def make(name, **kw):
    from piml_amd.scenarios import SCENARIOS
    return SCENARIOS[name](**kw).to(DEV)


def schedule(sc, seed, T):
    """(frame of each ordinal, per-frame counts) of the scene's spawn stream (the numpy restatements)."""
    if sc.spawn_law == 'gc':
        return scenario_ref.schedule(seed, T, sc.n_initial, sc.poisson_thresholds())
    born, _, counts = scenario_synth_ref.schedule(seed, T, sc.n_initial, sc.poisson_thresholds(), sc.poisson_thresholds2())
    return born, counts


def bits(x):
    """bit patterns (NaN-safe bitwise comparison)"""
    return x.view(torch.int32) if x.dtype == torch.float32 else x


BUFFERS = ('p', 'v', 'a', 'dest', 'hist', 'selff', 'desired_speed', 'mask', 'flag', 'waypoints', 'exit_idx', 'spawn_iters',
           'p_res', 'v_res', 'a_res', 'dest_res', 'mask_res', 'spawn_count', 'spawned', 'dropped')


@pytest.mark.parametrize('name', SCENES)
def test_members_are_bitwise_the_single_scene_frame(name):
    from piml_amd import ops_scenario
    sc = make(name, uniform_desired_speed=False)
    T = 201
    totals = [len(schedule(sc, s, T)[0]) for s in SEEDS]
    if max(totals) > min(totals):
        cap = min(totals)                # the first member to reach it keeps every agent, the others drop some
    else:                                # the square has no arrivals: every member holds 4 d^2 agents, all drop 3
        cap = totals[0] - 3
    hw = 4
    ens = ops_scenario.scenario_state(sc, cap, T, hist_width=hw, seeds=SEEDS)
    one = [ops_scenario.scenario_state(sc, cap, T, hist_width=hw, seed=s) for s in SEEDS]
    ops_scenario.scenario_step(ens, init=True)
    for st in one:
        ops_scenario.scenario_step(st, init=True)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    for _ in range(T - 1):
        rows = (torch.rand(len(SEEDS), cap, 2, device=DEV, generator=gen) * 4 - 2).contiguous()    # bounded, |a| <= 2
        ops_scenario.scenario_step(ens, rows)
        ens.t.add_(1)
        for m, st in enumerate(one):
            ops_scenario.scenario_step(st, rows[m].contiguous())
            st.t.add_(1)
    torch.cuda.synchronize()
    dropped = ens.dropped.tolist()
    assert dropped == [max(0, n - cap) for n in totals]
    if name != 'four_directional_square':
        assert min(dropped) == 0 < max(dropped)
    for m, st in enumerate(one):
        for k in BUFFERS:
            x, y = getattr(ens, k)[m], getattr(st, k)
            if k == 'dropped':                               # (S) against (1)
                x = x.reshape(1)
            assert x.shape == y.shape and torch.equal(bits(x), bits(y)), (name, m, k)


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


FIELDS = ('position', 'velocity', 'acceleration', 'destination', 'mask_p', 'waypoints', 'desired_speed', 'spawn_count')


def _same(a, b, fields=FIELDS):
    return all(torch.equal(bits(getattr(a, k).contiguous()), bits(getattr(b, k).contiguous())) for k in fields) and \
        a.spawned == b.spawned and a.dropped == b.dropped


def _row_invariant(sim, ens):
    """Does the network give a row the same bits inside the ensemble's S * cap rows as inside its member's cap rows?
    (one frame, the ensemble's last features as input, as the simulator calls it)"""
    st = ens.state
    S, cap = st.pf.shape[0], st.pf.shape[1]
    flat = lambda x: x.reshape(S * cap, *x.shape[2:])
    out = sim._in_scenario_mode(lambda: sim.model(flat(st.pf), flat(st.of), flat(st.selff))[0].reshape(S, cap, 2).clone())
    for m in range(S):
        own = sim._in_scenario_mode(lambda: sim.model(st.pf[m].contiguous(), st.of[m].contiguous(),
                                                      st.selff[m].contiguous())[0].clone())
        if not torch.equal(bits(out[m]), bits(own)):
            return False
    return True


@pytest.mark.parametrize('name', ['gc', 'crosswalk'])
def test_simulate_ensemble_end_to_end(sim, name):
    from piml_amd import ops
    sc = make(name)
    seeds, T = [5, 6, 9], 120
    g = sim.simulate_ensemble(sc, T, seeds, use_graph=True)
    e = sim.simulate_ensemble(sc, T, seeds, use_graph=False)
    g2 = sim.simulate_ensemble(sc, T, seeds)
    assert _same(g, e) and _same(g, g2)
    assert g.seeds == seeds and len(g) == 3 and g.position.shape[:2] == (3, T)
    for m, s in enumerate(seeds):
        born, counts = schedule(sc, s, T)
        assert np.array_equal(g.spawn_count[m].cpu().numpy(), counts) and g.spawned[m] == len(born) and g.dropped[m] == 0
    # the recorded features of the last frame are each member's own (members never see each other)
    a, st, t = sim.args, g.state, T - 1
    for m in range(3):
        pf, of, df = ops.relative_features(g.position[m, t], g.velocity[m, t], g.acceleration[m, t], g.destination[m, t],
                                           g.obstacles, a.topk_ped, a.sight_angle_ped, a.dist_threshold_ped, a.topk_obs,
                                           a.sight_angle_obs, a.dist_threshold_obs)
        for x, y in ((pf, st.pf[m]), (of, st.of[m]), (df, st.selff[m, :, :2])):
            assert torch.equal(torch.nan_to_num(x, 1e30), torch.nan_to_num(y, 1e30)), m
    # member m against the single simulation of its seed
    invariant = _row_invariant(sim, g)
    for m, s in enumerate(seeds):
        one = sim.simulate_scenario(sc, T, seed=s, capacity=g.capacity)
        mem = g.member(m)
        if invariant:
            assert _same(mem, one), m
        else:                            # frame 1 (the network's first output) agrees within 1e-6
            for k in ('position', 'velocity', 'acceleration'):
                x, y = getattr(mem, k)[:2], getattr(one, k)[:2]
                assert torch.equal(x.isnan(), y.isnan())
                assert (torch.nan_to_num(x) - torch.nan_to_num(y)).abs().max().item() <= 1e-6, (m, k)
    print(f'[ensemble] {name}: network rows invariant under the row count: {invariant}')


def test_collision_counts_per_member(sim):
    from piml_amd.functions import metrics
    ens = sim.simulate_ensemble(make('gc'), 80, [1, 2, 3, 4])
    for thr in (0.5, 0.25):
        counts = ens.collision_counts(thr)
        assert len(counts) == 4
        for m in range(4):
            mem = ens.member(m)
            want = metrics.collision_count(mem.position[:, :mem.num_agents], thr, reduction='sum')
            assert counts[m] == want, (thr, m)


def test_member_round_trip_and_pattern(sim, tmp_path):
    from piml_amd.data.data import RawData
    ens = sim.simulate_ensemble(make('gc'), 100, [3, 8])
    with pytest.raises(ValueError):
        ens.save_data(str(tmp_path / 'clip.npy'))
    paths = ens.save_data(str(tmp_path / 'clip_{seed}.npy'))
    assert paths == [str(tmp_path / 'clip_3.npy'), str(tmp_path / 'clip_8.npy')]
    for m, path in enumerate(paths):
        mem = ens.member(m)
        n = mem.num_agents
        raw = RawData()
        raw.load_trajectory_data(path)
        Tr = raw.num_steps
        mask = mem.mask_p[:Tr, :n].cpu().numpy()
        assert raw.num_pedestrians == n and np.array_equal(raw.mask_p.numpy(), mask)
        assert np.array_equal(raw.position.numpy()[mask == 1], mem.position[:Tr, :n].cpu().numpy()[mask == 1])
        assert torch.equal(mem.to_raw_data().mask_p, mem.mask_p[:, :n].cpu())


def test_simulate_cli_seeds(tmp_path):
    from piml_amd.data.data import RawData
    env = dict(os.environ, PYTHONPATH=REPO)
    out = str(tmp_path / 'clip_{seed}.npy')
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:3', '--frames', '40', '--out', out],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count('[simulate] gc (seed ') == 3 and 'mean +- std' in p.stdout
    for s in range(3):
        raw = RawData()
        raw.load_trajectory_data(out.replace('{seed}', str(s)))
        assert raw.num_pedestrians >= 20
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--seeds', '0:3', '--frames', '40',
                        '--out', str(tmp_path / 'clip.npy')], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0


def test_errors(sim):
    from piml_amd import _lib, ops_scenario
    from piml_amd.scenarios import gc_scenario
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.scenario_state(gc_scenario(), 64, 10, seeds=[1, 2])          # a CPU scenario
    with pytest.raises(ValueError):
        sim.simulate_ensemble(make('gc'), 10, [])
    with pytest.raises(ValueError):
        ops_scenario.scenario_state(make('gc'), 64, 10, seeds=[])
    st = ops_scenario.scenario_state(make('gc'), 64, 10, seeds=[1, 2])
    ops_scenario.scenario_step(st, init=True)
    for shape in ((64, 2), (3, 64, 2), (2, 63, 2)):
        with pytest.raises(ValueError):
            ops_scenario.scenario_step(st, torch.zeros(shape, device=DEV))
