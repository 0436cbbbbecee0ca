"""GPU: one MLAPM law per ensemble member (piml_scenario_step_mlapm_laws, MLAPM.simulate_sweep) and the fit of the law to
crowd statistics built on it (calibrate.calibrate_mlapm_to_stats): members bitwise their single-law runs, the edges of the
grid, the table read per launch under a captured graph, the entries' checks, statistics by candidate, the objective of the
truth, a twin experiment and the two command lines."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from test_scenario_clip_gpu import scene as clip_scene
from test_scenario_mlapm_gpu import FIELDS, LAW, SEEDS, _same, bits, make

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# three laws that differ in every constant, theta included
LAWS = [dict(LAW), dict(tau=0.6, A=6.0, B=-2.5, C=0.25, D=-0.2, theta=40.0),
        dict(tau=0.45, A=9.0, B=-3.5, C=0.1, D=-0.4, theta=70.0)]
SWEEPS = {'raw': [dict(version='raw', **p) for p in LAWS], 'GC': [dict(version='GC', **p) for p in LAWS],
          'UCY': [dict(version='UCY', **p) for p in LAWS],
          'mixed': [dict(version='raw', **LAWS[0]), dict(version='GC', **LAWS[1]), dict(version='UCY', radius=0.45, **LAWS[2])]}
UCY_CLIP = os.path.join(GOLDEN, 'data', 'UCY_Dataset_time162-216_timeunit0.08.npy')


def MLAPM():
    from piml_amd.models.mlapm import MLAPM as M
    return M


def single(params, sc, frames, seeds, capacity, radius=0.3):
    """the candidate's own single-law ensemble: MLAPM(**law).simulate_ensemble"""
    p = dict(params)
    radius = p.pop('radius', radius)
    return MLAPM()(**p).simulate_ensemble(sc, frames, seeds, capacity=capacity, radius=radius)


def assert_members_are_single_runs(sw, sc, frames, seeds):
    S = len(seeds)
    assert sw.n_candidates * S == len(sw) and sw.seeds_per_candidate == S and sw.seeds == list(seeds) * sw.n_candidates
    for c, params in enumerate(sw.params):
        one = single(params, sc, frames, seeds, sw.capacity)
        cand = sw.candidate(c)
        assert cand.seeds == list(seeds)
        for k in range(S):
            assert _same(sw.member(c * S + k), one.member(k)), (c, k)
            assert _same(cand.member(k), one.member(k)), (c, k)
            for f in FIELDS:                                                          # (as int32 bits, spelled out)
                a, b = getattr(sw, f)[c * S + k], getattr(one, f)[k]
                assert torch.equal(bits(a), bits(b)), (c, k, f)
        assert sw.spawned[c * S:(c + 1) * S] == one.spawned and sw.dropped[c * S:(c + 1) * S] == one.dropped


@pytest.mark.parametrize('kind', sorted(SWEEPS))
@pytest.mark.parametrize('name', ['gc', 'crosswalk', 'basic_unit3'])
def test_member_is_bitwise_its_single_run(name, kind):
    sc = make(name)
    sw = MLAPM().simulate_sweep(sc, 24, SWEEPS[kind], SEEDS)
    assert [p['version'] for p in sw.params] == [p['version'] for p in SWEEPS[kind]]
    assert_members_are_single_runs(sw, sc, 24, SEEDS)
    # the laws matter: two candidates of a seed share their arrivals and nothing else
    assert torch.equal(sw.spawn_count[0], sw.spawn_count[len(SEEDS)])
    assert not torch.equal(bits(sw.position[0]), bits(sw.position[len(SEEDS)]))


def test_one_candidate_is_the_single_law_run():
    sc = make('gc')
    p = dict(version='GC', **LAWS[1])
    sw = MLAPM().simulate_sweep(sc, 24, [p], SEEDS)
    ens = MLAPM()(**p).simulate_ensemble(sc, 24, SEEDS, capacity=sw.capacity)
    assert sw.n_candidates == 1 and all(_same(sw.member(m), ens.member(m)) for m in range(len(SEEDS)))
    for m, s in enumerate(SEEDS):
        assert _same(sw.member(m), MLAPM()(**p).simulate_scenario(sc, 24, seed=s, capacity=sw.capacity))


def test_capacity_not_a_multiple_of_the_block():
    sc = make('crosswalk')
    sw = MLAPM().simulate_sweep(sc, 24, SWEEPS['mixed'][1:], SEEDS[:2], capacity=27)     # 6 full agent blocks and 3 slots
    assert sw.capacity == 27 and max(sw.spawned) > 24
    assert_members_are_single_runs(sw, sc, 24, SEEDS[:2])


def test_sources_cross_the_lds_tile():
    """2056 agents in frame 0: the frame stages min(capacity, n + 64) = 2056 sources, one more tile than 2048"""
    n = 2056
    g = np.arange(n)
    table = np.zeros((n, 5, 2), np.float32)
    table[:, 0] = np.stack((0.9 * (g % 46), 0.9 * (g // 46)), 1)                       # a 46-wide grid, 0.9 m apart
    table[:, 1] = np.stack((np.where(g % 2, 1.0, -1.0), 0.3 * np.cos(g)), 1)            # moving, so that they see each other
    table[:, 2, 0] = 1.2 + 0.01 * (g % 7)
    table[:, 3] = np.stack((np.where(g % 2, 200.0, -200.0), 0.9 * (g // 46)), 1)
    table[:, 4] = np.nan
    sc = clip_scene(table, n_initial=n, rate=0.0, spawn_cap=0)
    laws = [SWEEPS['GC'][1], SWEEPS['UCY'][2]]
    sw = MLAPM().simulate_sweep(sc, 3, laws, [0], capacity=n)
    assert sw.spawned == [n, n] and int((sw.mask_p[:, 2] == 1).sum()) == 2 * n
    assert_members_are_single_runs(sw, sc, 3, [0])


def test_captured_table_is_read_on_every_launch():
    from piml_amd import hip_graphs_safe, ops_scenario, scenarios
    assert hip_graphs_safe()
    sc = make('crosswalk')
    seeds = SEEDS[:2] * 2
    rows = lambda ps: [ops_scenario.mlapm_law(p['version'], p['tau'], p['A'], p['B'], p['C'], p['D'], p['theta'],
                                              p.get('radius', 0.3)) for p in ps for _ in range(2)]
    first = ops_scenario.mlapm_law_table(rows(SWEEPS['mixed'][:2]), DEV)
    other = ops_scenario.mlapm_law_table(rows(SWEEPS['mixed'][1:]), DEV)
    assert first.shape == other.shape == (4, first.shape[1]) and not torch.equal(first, other)
    T = 9
    eager = scenarios.scenario_state_for(sc, T, 40, DEV, seeds=seeds)
    ops_scenario.scenario_step(eager, init=True)
    for t in range(T - 1):
        ops_scenario.scenario_step_mlapm(eager, first if t < 4 else other)
    st = scenarios.scenario_state_for(sc, T, 40, DEV, seeds=seeds)
    table = first.clone()
    ops_scenario.scenario_step(st, init=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(4):
            ops_scenario.scenario_step_mlapm(st, table, frame_offset=k, advance=False)
        st.t.add_(4)
    # (the capture ran nothing: the state is still frame 0's)
    assert int(st.t.item()) == 0
    graph.replay()
    table.copy_(other)                                   # in place: the same buffer the graph's launches point at
    graph.replay()
    torch.cuda.synchronize()
    assert int(st.t.item()) == int(eager.t.item()) == 8
    for a, b in ((st.p_res, eager.p_res), (st.v_res, eager.v_res), (st.a_res, eager.a_res), (st.dest_res, eager.dest_res),
                 (st.mask_res, eager.mask_res), (st.spawn_count, eager.spawn_count), (st.spawned, eager.spawned),
                 (st.p, eager.p), (st.v, eager.v)):
        assert torch.equal(bits(a), bits(b))
    # and the switch is visible: all eight frames under the first table end elsewhere
    same = scenarios.scenario_state_for(sc, T, 40, DEV, seeds=seeds)
    ops_scenario.scenario_step(same, init=True)
    for t in range(T - 1):
        ops_scenario.scenario_step_mlapm(same, first)
    assert not torch.equal(bits(same.p_res), bits(st.p_res))


def test_entries_reject_bad_arguments():
    from piml_amd import _lib, ops_scenario, scenarios
    L = _lib.lib()
    good = ops_scenario.mlapm_law()
    row = L.piml_mlapm_law_table_bytes(1)
    cases = [('variant', 3), ('variant', -1), ('tau', 0.0), ('tau', -1.0), ('radius', 0.0), ('radius', -0.3)]
    for field in ('tau', 'A', 'B', 'C', 'D', 'theta_deg', 'radius'):
        cases += [(field, float('nan')), (field, float('inf'))]
    for field, val in cases:
        arr = (_lib.MlapmLaw * 2)(_lib.MlapmLaw.from_buffer_copy(good), _lib.MlapmLaw.from_buffer_copy(good))
        setattr(arr[1], field, val)
        buf = (ctypes.c_ubyte * (2 * row))(*([0x5A] * (2 * row)))
        assert L.piml_mlapm_law_table_fill(arr, 2, buf) == 1, (field, val)
        assert bytes(buf) == b'\x5a' * (2 * row), (field, val)
    sc = make('gc')
    st = scenarios.scenario_state_for(sc, 10, 64, DEV, seeds=[1, 2])
    ops_scenario.scenario_step(st, init=True)
    table = ops_scenario.mlapm_law_table([good, good], DEV)
    torch.cuda.synchronize()
    before = [x.clone() for x in (st.p, st.v, st.p_res, st.spawned, st.t)]
    call = lambda tb=table.data_ptr(), members=2, off=0: L.piml_scenario_step_mlapm_laws(
        ctypes.byref(st.desc), None, members, st.seeds.data_ptr(), tb, off, None)
    assert call(tb=None) == 1 and call(members=0) == 1 and call(members=65536) == 1 and call(off=-1) == 1
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(before, (st.p, st.v, st.p_res, st.spawned, st.t)))
    for bad in (ops_scenario.mlapm_law_table([good], DEV), ops_scenario.mlapm_law_table([good] * 3, DEV), table.cpu(),
                table.view(-1), table.to(torch.int8)):
        with pytest.raises(ValueError):
            ops_scenario.scenario_step_mlapm(st, bad)
    with pytest.raises(TypeError):
        ops_scenario.scenario_step_mlapm(st, [good, good])
    sweep = MLAPM().simulate_sweep
    p = dict(version='GC', **LAW)
    for params, seeds in (([], [0]), ([p], []), ([dict(p, E=1.0)], [0]), ([dict(p, theta_deg=1.0)], [0]),
                          ([{k: v for k, v in p.items() if k != 'tau'}], [0]), ([p] * 256, range(256)),
                          ([dict(p, tau=0.0)], [0]), ([dict(p, radius=-1.0)], [0])):
        with pytest.raises(ValueError):
            sweep(sc, 10, params, seeds)
    assert call() == 0                                   # the state is still good for a frame
    torch.cuda.synchronize()


# ---- statistics by candidate, the objective and the search ----------------------------------------------------------

TRUTH = dict(version='GC', **LAW)                        # tau = 0.5
OFF = dict(TRUTH, tau=1.0)
SEEDS4 = [0, 1, 2, 3]
CROWD_KW = dict(box=(-13.0, 13.0, -11.0, 11.0), cell=1.0)
PAIR_KW = dict(lags=(16, 32))


@pytest.fixture(scope='module')
def twin():
    """the crosswalk under TRUTH for 64 frames of 4 seeds, its pooled statistics, and the sweep of [TRUTH, OFF]"""
    sc = make('crosswalk')
    ens = MLAPM()(**TRUTH).simulate_ensemble(sc, 64, SEEDS4)
    ref = (ens.crowd_stats(**CROWD_KW).pooled(), ens.pair_stats(**PAIR_KW).pooled())
    sw = MLAPM().simulate_sweep(sc, 64, [TRUTH, OFF], SEEDS4)
    return sc, ref, sw, sw.crowd_stats(**CROWD_KW), sw.pair_stats(**PAIR_KW)


def test_statistics_by_candidate(twin):
    from piml_amd import crowdstats, pairstats
    _, _, sw, crowd, pairs = twin
    assert crowd.members == pairs.members == 8
    for c in range(2):
        group = sw.members_of(c)
        assert group == list(range(4 * c, 4 * c + 4))
        cand = sw.candidate(c)
        want_c, got_c = cand.crowd_stats(**CROWD_KW).pooled(), crowd.select(group).pooled()
        for k in crowdstats.ARRAYS:
            assert np.array_equal(getattr(got_c, k), getattr(want_c, k)), (c, k)
        want_p, got_p = cand.pair_stats(**PAIR_KW).pooled(), pairs.select(group).pooled()
        for k in pairstats.ARRAYS:
            assert np.array_equal(getattr(got_p, k), getattr(want_p, k)), (c, k)
        assert got_c.options == want_c.options and got_p.options == want_p.options
    assert int(crowd.select(sw.members_of(0)).pooled().n.sum()) > 2000


def test_objective_of_the_truth_is_zero(twin):
    from piml_amd.calibrate import stats_objective
    _, (ref_c, ref_p), sw, crowd, pairs = twin
    J = []
    for c in range(2):
        g = sw.members_of(c)
        j, terms = stats_objective(crowd.select(g).pooled(), pairs.select(g).pooled(), ref_c, ref_p)
        print(f'[sweep] candidate {c}: J = {j:.6g}, terms {terms}')
        assert terms['map_distance'] is not None and (c or terms['fd_bins'] >= 1)
        J.append(j)
    assert J[0] == 0.0 and J[1] > 0.0


def test_twin_experiment_recovers_tau(twin):
    from piml_amd.calibrate import PARAM_NAMES, calibrate_mlapm_to_stats
    sc, ref, _, _, _ = twin
    init = {k: OFF[k] for k in PARAM_NAMES}
    res = calibrate_mlapm_to_stats(sc, ref, version='GC', init=init, fit=('tau',), frames=64, seeds=SEEDS4, population=8,
                                   generations=6)
    print(f'[sweep] twin experiment: tau {init["tau"]} -> {res.params["tau"]:.6g} (truth 0.5), J {res.initial_loss:.6g} -> '
          f'{res.final_loss:.6g}, history {res.history}, terms {res.terms}, seconds {getattr(res, "seconds", None)}')
    assert all(y <= x for x, y in zip(res.history, res.history[1:]))
    assert res.final_loss < res.initial_loss
    assert abs(res.params['tau'] - 0.5) < 0.5
    for k in PARAM_NAMES:
        if k != 'tau':
            assert np.float64(res.params[k]).tobytes() == np.float64(init[k]).tobytes(), k
    assert res.params['version'] == 'GC' and res.generations == 6 and res.population == 8 and res.seeds == SEEDS4
    assert res.fit == ('tau',) and set(res.terms) >= {'fd_distance', 'ttc_l1', 'nn_l1', 'overlap_rate_diff'}


# ---- command lines --------------------------------------------------------------------------------------------------

def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m'] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_simulate_cli_params_sweep(tmp_path):
    files = []
    for c, p in enumerate((TRUTH, OFF)):
        files.append(str(tmp_path / f'law{c}.json'))
        with open(files[-1], 'w') as fh:
            json.dump(p, fh)
    out = str(tmp_path / 'sweep.json')
    text = _run(['piml_amd.simulate', '--law', 'mlapm', '--params-sweep', *files, '--scenario', 'crosswalk', '--seeds', '0:2',
                 '--frames', '40', '--stats', out])
    assert text.count('[simulate] crosswalk candidate ') == 2
    got = json.load(open(out))
    assert got['seeds'] == [0, 1] and len(got['candidates']) == 2
    for c, entry in enumerate(got['candidates']):
        assert entry['params']['tau'] == (TRUTH, OFF)[c]['tau'] and entry['file'] == files[c]
        assert len(entry['stats']['arrays']['n']) == 1                                # pooled over the candidate's seeds
    from piml_amd import simulate
    for bad in (['--law', 'mlapm', '--params-sweep', files[0], '--params', files[1], '--seeds', '0:2', '--stats', out],
                ['--law', 'mlapm', '--params-sweep', files[0], '--stats', out],
                ['--params-sweep', files[0], '--seeds', '0:2', '--stats', out],
                ['--law', 'mlapm', '--params-sweep', files[0], '--seeds', '0:2', '--out', str(tmp_path / 'x_{seed}.npy')]):
        with pytest.raises(SystemExit):
            simulate.get_args(bad)


def test_calibrate_cli_match_stats(tmp_path):
    out = str(tmp_path / 'params.json')
    text = _run(['piml_amd.calibrate', '--data', UCY_CLIP, '--version', 'UCY', '--match-stats', '--scene-frames', '100:140',
                 '--population', '4', '--generations', '2', '--seeds', '0:2', '--fit', 'tau,A', '--out', out])
    assert 'objective' in text and '[calibrate] terms:' in text and 'wrote' in text
    got = json.load(open(out))
    assert sorted(got) == sorted(['version', 'tau', 'A', 'B', 'C', 'D', 'theta']) and got['version'] == 'UCY'
    from piml_amd import simulate
    assert simulate.load_mlapm_params(out) == got
