"""No GPU: the exit choice (piml_nav_choose_exit; ops_scenario.exit_choice_law / nav_choose_exit; MLAPM.simulate_*(...,
exit_choice=); simulate --exit-choice).  Properties of the restatement (tests/navchoice_ref.py) that the GPU tests compare the
kernel with, the header's declaration and its binding, every refusal of the entry that returns before any HIP call, the Python
and command-line refusals, the plan's "exits" key, and the new kernel's resource use read from the library."""
import ctypes
import dataclasses
import json
import os
import re

import numpy as np
import pytest

import nav_ref
import navchoice_cases as CASES
import navchoice_ref as REF
import scenario_ref
from conftest import REPO
from test_navfield import BAD_NAVS, PLAN, _fake_nav, _fake_scene

f32 = np.float32
INF = f32(np.inf)


# ---- 1. the restatement ----

def _hall(cap=120, seed=5):
    """an empty 33 x 34 grid of 0.5 m cells with three gates in one class, well apart, and `cap` agents as the spawn wrote
    them (scenario_ref.spawn_agents: waypoints (d, d), exit_idx the entry nearest d), standing at random cells"""
    gx, gy, cell, x0, y0 = 33, 34, 0.5, 0.0, 0.0
    blocked = np.zeros((gy, gx), np.uint8)
    goal = np.zeros((3, gy, gx), np.uint8)
    spots = [(2, 3), (30, 16), (5, 31)]
    entries = np.zeros((3, 4, 2), f32)
    for g, (x, y) in enumerate(spots):
        goal[g, y, x] = 1
        entries[g] = [(f32(x0 + (x + 0.2 + 0.2 * j) * cell), f32(y0 + (y + 0.5) * cell)) for j in range(4)]
    u, _ = nav_ref.solve(blocked, goal)
    o, d, _, dr = scenario_ref.spawn_agents(seed, np.arange(cap), entries, spawn_offset=0.8)
    ex = scenario_ref.nearest_entry(d, entries).astype(np.int32)
    assert np.array_equal(ex, dr['de'])                          # the gates are far enough apart: nearest(d) is the drawn gate
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(x0 + 0.01, x0 + gx * cell - 0.01, cap), rng.uniform(y0 + 0.01, y0 + gy * cell - 0.01, cap)], -1)
    state = dict(p=p.astype(f32), dest=d.copy(), flag=np.zeros(cap, np.int32), mask=np.ones(cap, f32),
                 waypoints=np.stack([d, d]).astype(f32), exit_idx=np.stack([ex, ex]), n=cap)
    return state, u, entries, dr, (x0, y0, cell), seed


def _same_state(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32) if np.asarray(a[k]).dtype == f32 else np.asarray(a[k]),
                              np.asarray(b[k]).view(np.uint32) if np.asarray(b[k]).dtype == f32 else np.asarray(b[k]))
               for k in a)


def test_an_infinite_margin_changes_nothing():
    state, u, entries, dr, (x0, y0, cell), seed = _hall()
    cls = REF.gate_class([[0, 1, 2]], 3)
    new, sw = REF.choose(state, u, x0, y0, cell, cls, INF, f32(0), 8, 9, seed, entries, 0.8)
    assert sw.sum() == 0 and _same_state(new, state)
    # and so does a frame that is not scheduled, whatever the margin
    for t in (0, 8, 10):
        new, sw = REF.choose(state, u, x0, y0, cell, cls, f32(0), f32(0), 8, t, seed, entries, 0.8)
        assert sw.sum() == 0 and _same_state(new, state), t
    new, sw = REF.choose(state, u, x0, y0, cell, cls, f32(0), f32(0), 8, 1, seed, entries, 0.8)
    assert sw.sum() > 0                                          # t = 1 is the first scheduled frame


def test_with_no_margin_every_agent_is_bound_for_the_least_u_of_the_gates_it_did_not_enter_by():
    state, u, entries, dr, (x0, y0, cell), seed = _hall()
    cls = REF.gate_class([[0, 1, 2]], 3)
    new, sw = REF.choose(state, u, x0, y0, cell, cls, f32(0), f32(0), 8, 9, seed, entries, 0.8)
    assert 10 < sw.sum() < len(sw)
    for i in range(len(sw)):
        cx, cy = REF.cell_of(state['p'][i], x0, y0, cell, 33, 34)
        col = u[:, cy, cx]
        others = [g for g in range(3) if g != dr['oe'][i]]
        least = min(others, key=lambda g: (col[g], g))
        got = int(new['exit_idx'][0, i])
        assert col[got] == col[least] and got != dr['oe'][i], (i, got, least, col)
        assert got == int(new['exit_idx'][1, i])
        # the destination is the spawn's for that gate: the same point index and offset
        want = (entries[got, dr['di'][i]] + dr['ud'][i] * f32(0.8)).astype(f32)
        assert np.array_equal(new['dest'][i].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(new['waypoints'][:, i].view(np.uint32), np.stack([want, want]).view(np.uint32))
    # a second pass on the result changes nothing more
    again, sw2 = REF.choose(new, u, x0, y0, cell, cls, f32(0), f32(0), 8, 17, seed, entries, 0.8)
    assert sw2.sum() == 0 and _same_state(again, new)


def test_a_switch_back_restores_the_state_bit_for_bit():
    state, u, entries, dr, (x0, y0, cell), seed = _hall()
    cls = REF.gate_class([[0, 1, 2]], 3)
    away = u.copy()                                              # a field under which every agent's own gate reads worst
    for i in range(len(state['mask'])):
        cx, cy = REF.cell_of(state['p'][i], x0, y0, cell, 33, 34)
        away[:, cy, cx] = f32(10)
    back = away.copy()
    for i in range(len(state['mask'])):
        cx, cy = REF.cell_of(state['p'][i], x0, y0, cell, 33, 34)
        if (away[:, cy, cx] == f32(10)).all():                   # (agents that share a cell follow its first agent)
            away[state['exit_idx'][0, i], cy, cx] = f32(50)
            back[:, cy, cx] = f32(50)
            back[state['exit_idx'][0, i], cy, cx] = f32(10)
    there, sw = REF.choose(state, away, x0, y0, cell, cls, f32(1), f32(0), 8, 9, seed, entries, 0.8)
    home, sw2 = REF.choose(there, back, x0, y0, cell, cls, f32(1), f32(0), 8, 17, seed, entries, 0.8)
    both = (sw == 1) & (sw2 == 1) & (home['exit_idx'][0] == state['exit_idx'][0])
    assert both.sum() > 50
    assert not np.array_equal(there['dest'][both], state['dest'][both])
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32) if x.dtype == f32 else x
    assert np.array_equal(bits(home['dest'][both]), bits(state['dest'][both]))
    assert np.array_equal(bits(home['waypoints'][:, both]), bits(state['waypoints'][:, both]))
    assert np.array_equal(home['exit_idx'][:, both], state['exit_idx'][:, both])


def test_every_case_of_the_rule_is_in_the_shared_state():
    """the state the GPU tests run holds each case, and the restatement decides each as the rule says"""
    for G in (3, 64):
        case = CASES.build(300, 3, G, 'ushape')
        new, sw = CASES.expected(case)
        idx, oe = case['case'], case['oe']
        C = CASES.classes_of(G)[0]
        cur0, best0 = C[0], C[-1]
        named = lambda name: idx == CASES.CASES.index(name)
        live = np.broadcast_to(np.arange(300)[None] < case['n'], idx.shape)
        free = live & (oe != best0) & (oe != cur0)               # slots whose origin gate is neither of the two gates at stake
        for name in ('all_unreachable', 'equal', 'at_margin', 'inside_commit', 'nan_position', 'outside', 'mask0', 'retired',
                     'cur_classless'):
            assert named(name).sum() >= 40 and sw[named(name)].sum() == 0, name
        for name in ('cur_unreachable', 'ulp_below_margin', 'flag1', 'tie_lowest', 'far_better'):
            assert (named(name) & free).sum() >= 10 and sw[named(name) & free].all(), name
        assert (~live).sum() == 6 and sw[~live].sum() == 0       # the slots not yet spawned hold live-looking data
        assert all(s['mask'][case['n']:].all() for s in case['states'])
        m, i = np.argwhere(named('flag1') & free)[0]
        assert new[m]['exit_idx'][0, i] == (1 if G == 3 else 63) and new[m]['exit_idx'][1, i] != cur0     # row 0 is not written
        assert np.array_equal(new[m]['waypoints'][0, i].view(np.uint32), case['states'][m]['waypoints'][0, i].view(np.uint32))
        # the origin gate reads lowest and is passed over
        on = named('origin_nearest') & live
        hit = [(m, i) for m, i in np.argwhere(on) if case['u'][m, oe[m, i]][tuple(
            REF.cell_of(case['states'][m]['p'][i], CASES.X0, CASES.Y0, CASES.CELL, case['gx'], case['gy'])[::-1])] == f32(0.5)]
        assert len(hit) >= 3
        assert all(new[m]['exit_idx'][1, i] != oe[m, i] for m, i in hit)
        if G == 64:
            m, i = np.argwhere(named('tie_lowest') & free & (oe != C[1]))[0]
            assert new[m]['exit_idx'][1, i] != best0 and sw[m, i]    # gates 1 and 31 tie: the lower index wins
        # nothing is written past row 1
        assert all(np.isnan(s['waypoints'][2]).all() for s in new)


# ---- 2. the header, the binding, the entry's refusals ----

def test_header_declares_and_lib_binds_the_entry():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint piml_nav_choose_exit\s*\(', text) and 'typedef struct piml_exit_choice' in text
    assert len(_lib.SIGNATURES['piml_nav_choose_exit']) == 10 and hasattr(_lib.lib(), 'piml_nav_choose_exit')
    assert [f for f, _ in _lib.ExitChoice._fields_] == ['margin', 'commit', 'every'] and ctypes.sizeof(_lib.ExitChoice) == 12
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # a symbol and a struct were only added


def _law(margin=1.0, commit=2.0, every=8):
    from piml_amd import _lib
    d = _lib.ExitChoice()
    d.margin, d.commit, d.every = margin, commit, every
    return d


def test_entry_refuses_bad_arguments_without_gpu():
    """every call is refused: the argument set that passes (launched in test_navchoice_gpu.py) differs from each in one thing"""
    from piml_amd import _lib
    L = _lib.lib()
    s, nav = _fake_scene(), _fake_nav()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    buf = ctypes.addressof(nav._keep)
    keep = dict(s_=s, members=1, seeds_=seeds, nav_=nav, stride=0, cls=buf, law=_law(), count=None, offset=0)

    def call(**kw):
        k = dict(keep, **kw)
        opt = lambda x: None if x is None else ctypes.byref(x)
        return L.piml_nav_choose_exit(opt(k['s_']), k['members'], k['seeds_'], opt(k['nav_']), k['stride'], k['cls'],
                                      opt(k['law']), k['count'], k['offset'], None)
    nan, inf = float('nan'), float('inf')
    assert call(s_=None) == 1 and call(nav_=None) == 1 and call(cls=None) == 1 and call(law=None) == 1
    # the frame's own checks
    assert call(s_=_lib.Scenario()) == 1 and call(members=0) == 1 and call(members=65536) == 1
    assert call(s_=_fake_scene(capacity=0)) == 1 and call(s_=_fake_scene(position=None)) == 1
    assert call(s_=_fake_scene(exit_idx=None)) == 1 and call(s_=_fake_scene(frame_counter=None)) == 1
    assert call(seeds_=None, members=2) == 1
    # the grid, and the scene against it
    for kw in BAD_NAVS:
        assert call(nav_=_fake_nav(**kw)) == 1, kw
    assert call(nav_=_fake_nav(G=3)) == 1 and call(s_=_fake_scene(E=3)) == 1
    assert call(s_=_fake_scene(route_max_iters=1)) == 1 and call(s_=_fake_scene(route_max_iters=16)) == 1
    assert call(s_=_fake_scene(D=1)) == 1
    # the law, the stride, the offset
    assert call(law=_law(every=0)) == 1 and call(law=_law(every=-8)) == 1
    assert call(law=_law(margin=-0.5)) == 1 and call(law=_law(margin=nan)) == 1 and call(law=_law(margin=-inf)) == 1
    assert call(law=_law(commit=-0.5)) == 1 and call(law=_law(commit=nan)) == 1
    assert call(stride=-1) == 1 and call(offset=-1) == 1


def test_the_kernel_builds_for_gfx950_without_scratch():
    pytest.importorskip('msgpack')
    from piml_amd import _lib
    usage = _lib.kernel_resource_usage()
    name = 'scenario_choose_exit_kernel'
    assert name in usage, sorted(k for k in usage if 'scenario' in k)
    assert usage[name]['vgpr_spill'] == 0 and usage[name]['sgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, usage[name]
    assert usage[name]['lds_bytes'] == 0


# ---- 3. Python ----

def test_exit_choice_law_is_checked():
    from piml_amd import ops_scenario
    law = ops_scenario.exit_choice_law([[1, 2], (3, 4, 5)])
    assert law.classes == ((1, 2), (3, 4, 5)) and (law.margin, law.commit, law.every) == (1.0, 2.0, 8)
    assert law.gate_class_host(7) == [-1, 0, 0, 1, 1, 1, -1]
    d = law.desc(0.25)
    assert (d.margin, d.commit, d.every) == (4.0, 8.0, 8)
    third = ops_scenario.exit_choice_law([[0, 1]], margin=1.0, commit=0.0).desc(0.3)
    assert third.margin == float(f32(1.0) / f32(0.3)) and third.commit == 0.0     # divided in float32
    assert ops_scenario.exit_choice_law([[0, 1]], margin=float('inf')).desc(0.25).margin == float('inf')
    with pytest.raises(ValueError, match='outside'):
        law.gate_class_host(5)                                   # the index meets a scene of five gates
    for bad in ([[1]], [[1, 2], [2, 3]], [[1, 1]], [[-1, 2]], [], [[]], 'ab', [[1.5, 2]], None, [[1, 2], 3]):
        with pytest.raises(ValueError):
            ops_scenario.exit_choice_law(bad)
    for kw in (dict(margin=-1.0), dict(margin=float('nan')), dict(commit=-0.1), dict(commit=float('nan')), dict(every=0),
               dict(every=2.5), dict(every=True), dict(every=-8)):
        with pytest.raises(ValueError):
            ops_scenario.exit_choice_law([[1, 2]], **kw)


def test_floorplan_exits_and_the_plan_key(tmp_path):
    from piml_amd import scenarios
    gates = PLAN['gates'] + [[[10.0, 7.0], [10.0, 9.5]]]
    sc = scenarios.floorplan_scenario(PLAN['walls'], gates, exits=[[1, 2]])
    assert sc.exit_classes == [[1, 2]] and sc.to('cpu').exit_classes == [[1, 2]]
    assert scenarios.floorplan_scenario(PLAN['walls'], gates).exit_classes is None
    assert scenarios.gc_scenario().exit_classes is None
    for bad in ([[1]], [[1, 3]], [[0, 1], [1, 2]], 'x'):
        with pytest.raises(ValueError, match='exits'):
            scenarios.floorplan_scenario(PLAN['walls'], gates, exits=bad)
    with pytest.raises(ValueError):
        scenarios.floorplan_scenario(PLAN['walls'], gates, exit_classes=[[1, 2]])        # the field is set through exits=
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(walls=PLAN['walls'], gates=gates, exits=[[2, 1]], n_initial=3)))
    got = scenarios.load_floorplan(str(path))
    assert got.exit_classes == [[2, 1]] and got.n_initial == 3
    path.write_text(json.dumps(dict(walls=PLAN['walls'], gates=gates, exits=[[1, 5]])))
    with pytest.raises(ValueError, match='exits'):
        scenarios.load_floorplan(str(path))


def test_runs_an_exit_choice_cannot_join_are_refused_before_any_state():
    """on the CPU: every refusal speaks before scenario_state would ask for a GPU"""
    import torch
    from piml_amd import ops_scenario, scenarios
    from piml_amd.models.mlapm import MLAPM, SweepRun
    from test_navfield import BASE
    gates = PLAN['gates'] + [[[10.0, 7.0], [10.0, 9.5]]]
    sc = scenarios.floorplan_scenario(PLAN['walls'], gates, exits=[[1, 2]])
    bare = scenarios.floorplan_scenario(PLAN['walls'], gates)
    law = ops_scenario.exit_choice_law([[1, 2]])
    m = MLAPM(**BASE)
    with pytest.raises(ValueError, match='needs nav'):
        m.simulate_scenario(sc, 5, exit_choice=True)
    with pytest.raises(ValueError, match='needs nav'):
        m.simulate_ensemble(sc, 5, [0, 1], exit_choice=law)
    with pytest.raises(ValueError, match='needs nav'):
        MLAPM.simulate_sweep(sc, 5, [BASE], [0], exit_choice=law)
    with pytest.raises(ValueError, match='exit_classes'):
        m.simulate_scenario(bare, 5, nav=True, exit_choice=True)
    with pytest.raises(ValueError, match='outside'):
        m.simulate_scenario(sc, 5, nav=True, exit_choice=ops_scenario.exit_choice_law([[1, 3]]))
    with pytest.raises(TypeError):
        m.simulate_scenario(sc, 5, nav=True, exit_choice=[[1, 2]])
    with pytest.raises(TypeError):
        SweepRun(sc, 5, 1, [0], nav=True, exit_choice='yes')
    with pytest.raises(ValueError, match='grouped'):
        m.simulate_scenario(dataclasses.replace(sc, spawn_law='clip_groups'), 5, nav=True, exit_choice=law)
    with pytest.raises(ValueError, match='route_max_iters'):
        m.simulate_scenario(scenarios.gc_scenario(), 5, nav=True, exit_choice=ops_scenario.exit_choice_law([[3, 4]]))
    # False and None are no choice: the run gets as far as asking for a GPU state
    assert ops_scenario.resolve_exit_choice(sc, None, None) is None and ops_scenario.resolve_exit_choice(sc, False, None) is None
    got = ops_scenario.resolve_exit_choice(sc, True, True)
    assert got.classes == ((1, 2),) and (got.margin, got.commit, got.every) == (1.0, 2.0, 8)
    assert ops_scenario.resolve_exit_choice(sc, law, 'sight') is law
    # the network-driven simulator
    from piml_amd.models.simulators import BaseSimulator
    from test_simulator_gpu import sim_args
    sim = BaseSimulator(sim_args(device='cpu'))
    sim.model.eval()
    with pytest.raises(ValueError, match='needs nav'):
        sim.simulate_scenario(sc, 5, exit_choice=True)
    with pytest.raises(ValueError, match='exit_classes'):
        sim.simulate_ensemble(bare, 5, [0, 1], nav=True, exit_choice=True)
    with pytest.raises(TypeError):
        sim.simulate_scenario(sc, 5, nav=True, exit_choice=1.0)
    assert torch.is_grad_enabled()


def test_command_line(tmp_path):
    from piml_amd import simulate
    gates = PLAN['gates'] + [[[10.0, 7.0], [10.0, 9.5]]]
    plan = tmp_path / 'plan.json'
    plan.write_text(json.dumps(dict(walls=PLAN['walls'], gates=gates, exits=[[1, 2]], n_initial=4)))
    bare = tmp_path / 'bare.json'
    bare.write_text(json.dumps(dict(walls=PLAN['walls'], gates=gates, n_initial=4)))
    head = ['--law', 'mlapm', '--scene-plan', str(plan)]
    own, _ = simulate.get_args(head + ['--nav', '--exit-choice'])
    assert own.exit_law.classes == ((1, 2),) and (own.exit_law.margin, own.exit_law.commit, own.exit_law.every) == (1.0, 2.0, 8)
    own, _ = simulate.get_args(head + ['--nav', '--exit-choice', '--exit-classes', '2,1', '--exit-margin', '0.5', '--exit-commit',
                                       '3', '--exit-every', '16', '--nav-density', '2'])
    assert own.exit_law.classes == ((2, 1),) and (own.exit_law.margin, own.exit_law.commit, own.exit_law.every) == (0.5, 3.0, 16)
    own, _ = simulate.get_args(['--scene-plan', str(bare), '--route', 'sight', '--exit-choice', '--exit-classes', '1,2'])
    assert own.exit_law.classes == ((1, 2),) and own.law != 'mlapm'
    own, _ = simulate.get_args(['--law', 'mlapm', '--scenario', 'gc', '--nav', '--exit-choice', '--exit-classes', '3,4;1,2'])
    assert own.exit_law.classes == ((3, 4), (1, 2))
    own, _ = simulate.get_args(head + ['--nav'])
    assert own.exit_law is None and not own.exit_choice
    for argv in (head + ['--exit-choice'],                                        # no floor field
                 head + ['--nav', '--exit-classes', '1,2'], head + ['--nav', '--exit-margin', '1'],
                 head + ['--nav', '--exit-commit', '1'], head + ['--nav', '--exit-every', '8'],
                 ['--law', 'mlapm', '--scene-plan', str(bare), '--nav', '--exit-choice'],           # no classes anywhere
                 ['--law', 'mlapm', '--scenario', 'gc', '--nav', '--exit-choice'],
                 head + ['--nav', '--exit-choice', '--exit-classes', '1;2'], head + ['--nav', '--exit-choice', '--exit-classes', 'a,b'],
                 head + ['--nav', '--exit-choice', '--exit-classes', '1,3'],                         # a plan of three gates
                 ['--law', 'mlapm', '--scenario', 'gc', '--nav', '--exit-choice', '--exit-classes', '3,7'],
                 head + ['--nav', '--exit-choice', '--exit-margin', '-1'], head + ['--nav', '--exit-choice', '--exit-every', '0'],
                 ['--law', 'mlapm', '--scenario', 'crosswalk', '--exit-choice']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)
