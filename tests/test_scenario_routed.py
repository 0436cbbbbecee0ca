"""No GPU: the floor field under the network-driven frame (piml_scenario_step_nav; BaseSimulator.simulate_*(..., nav=);
simulate --route).  The header's declaration and its binding, the entry's refusals that return before any HIP call, the routed
kernels' resource use read from the library, the command line's --route flag, and the scenes a field cannot route refused
before any state exists."""
import ctypes
import dataclasses
import json
import os
import re

import pytest

from conftest import REPO
from test_navfield import BAD_NAVS, PLAN, _fake_nav, _fake_scene


def test_header_declares_and_lib_binds_the_entry():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint piml_scenario_step_nav\s*\(', text)
    assert len(_lib.SIGNATURES['piml_scenario_step_nav']) == 10 and hasattr(_lib.lib(), 'piml_scenario_step_nav')
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # a symbol was only added


def _fake_sight(nav, **kw):
    from piml_amd import _lib
    s = _lib.NavSight()
    s.parent, s.G, s.gx, s.gy = nav.u, nav.G, nav.gx, nav.gy
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_refuses_bad_arguments_without_gpu():
    """every call is refused: the argument set that passes (launched in test_scenario_routed_gpu.py) differs from each in one
    thing"""
    from piml_amd import _lib
    L = _lib.lib()
    s, nav = _fake_scene(), _fake_nav()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    buf = ctypes.addressof(nav._keep)
    keep = dict(s_=s, r=None, members=1, seeds_=seeds, a=buf, init=0, nav_=nav, sight=None, steer=buf)

    def call(**kw):
        k = dict(keep, **kw)
        opt = lambda x: None if x is None else ctypes.byref(x)
        return L.piml_scenario_step_nav(opt(k['s_']), opt(k['r']), k['members'], k['seeds_'], k['a'], k['init'], opt(k['nav_']),
                                        opt(k['sight']), k['steer'], None)
    # what piml_scenario_step_members refuses
    assert call(s_=None) == 1 and call(s_=_lib.Scenario()) == 1 and call(members=0) == 1 and call(members=65536) == 1
    assert call(a=None) == 1 and call(init=2) == 1 and call(init=-1) == 1
    assert call(s_=_fake_scene(capacity=0)) == 1 and call(s_=_fake_scene(position=None)) == 1
    assert call(s_=_fake_scene(exit_idx=None)) == 1 and call(s_=_fake_scene(D=9)) == 1
    # a single run may leave the seeds out, an ensemble may not
    assert call(seeds_=None, members=2) == 1 and call(seeds_=None, members=3) == 1
    # the field's own: a scene rule, a detour route, another number of gates, a bad grid, a bad table, no steer
    for law_name in ('crosswalk', 'square', 'unit1', 'clip'):
        r = _lib.ScenarioRules()
        r.spawn_law, r.arrival_rule = _lib.SPAWN_LAWS[law_name], _lib.ARRIVAL_RULES['radius']
        assert call(r=r) == 1, law_name
    r = _lib.ScenarioRules()
    r.spawn_law = _lib.SPAWN_CLIP_GROUPS
    assert call(r=r) == 1
    assert call(s_=_fake_scene(route_max_iters=1)) == 1 and call(s_=_fake_scene(route_max_iters=16)) == 1
    assert call(nav_=_fake_nav(G=3)) == 1 and call(s_=_fake_scene(E=3)) == 1 and call(nav_=None) == 1
    for kw in BAD_NAVS:
        assert call(nav_=_fake_nav(**kw)) == 1, kw
    for kw in (dict(parent=None), dict(G=3), dict(gx=5), dict(gy=4)):
        assert call(sight=_fake_sight(nav, **kw)) == 1, kw
    assert call(steer=None) == 1 and call(steer=None, init=1, a=None) == 1


def test_routed_kernels_do_not_spill():
    pytest.importorskip('msgpack')
    from piml_amd import _lib
    usage = _lib.kernel_resource_usage()
    for name in ('scenario_frame_nav_kernel<false>', 'scenario_frame_nav_kernel<true>'):
        assert name in usage, sorted(k for k in usage if 'scenario_frame' in k)
        assert usage[name]['vgpr_spill'] == 0 and usage[name]['scratch_bytes'] == 0, (name, usage[name])
        assert usage[name]['lds_bytes'] == usage['scenario_frame_kernel<true>']['lds_bytes']     # the staged entry points


def test_command_line_route(tmp_path, capsys):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, n_initial=4)))
    for law in ([], ['--law', 'pinnsf'], ['--law', 'mlapm']):
        for route in ('field', 'sight'):
            own, _ = simulate.get_args(law + ['--scenario', 'gc', '--route', route])
            assert own.route == route and own.routed and own.route_sight == (route == 'sight') and not own.nav
            assert own.nav_cell == 0.25 and own.nav_clearance == 0.3 and own.plan is None
            own, _ = simulate.get_args(law + ['--scene-plan', str(path), '--route', route, '--seeds', '0:2', '--obstacle-stats',
                                              str(tmp_path / 'o.json')])
            assert own.route == route and own.routed and own.plan.n_initial == 4 and own.plan.route_max_iters == 0
    own, _ = simulate.get_args(['--route', 'field', '--nav-cell', '0.125', '--nav-clearance', '0.4'])
    assert own.nav_cell == 0.125 and own.nav_clearance == 0.4
    # --nav keeps meaning what it meant, and says so in the same fields
    own, _ = simulate.get_args(['--law', 'mlapm', '--nav', '--nav-sight'])
    assert own.nav and own.route is None and own.routed and own.route_sight
    own, _ = simulate.get_args(['--law', 'mlapm'])
    assert not own.routed and not own.route_sight
    clip = str(tmp_path / 'clip.npy')
    for argv in (['--scenario', 'crosswalk', '--route', 'field'], ['--law', 'mlapm', '--scenario', 'crosswalk', '--route', 'sight'],
                 ['--scene-from', clip, '--route', 'field'], ['--law', 'mlapm', '--scene-from', clip, '--route', 'field'],
                 ['--law', 'mlapm', '--nav', '--route', 'field'], ['--law', 'mlapm', '--nav', '--nav-sight', '--route', 'sight'],
                 ['--route', 'yes'], ['--route'], ['--route', 'field', '--nav-sight'], ['--route', 'field', '--nav-cell', '0'],
                 ['--nav-cell', '0.5'], ['--law', 'pinnsf', '--nav'], ['--nav'], ['--law', 'pinnsf', '--scene-plan', str(path)],
                 ['--law', 'pinnsf', '--scene-plan', str(path), '--nav-sight']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'pinnsf', '--scene-plan', str(path)])
    err = capsys.readouterr().err
    assert 'floor field' in err and '--route' in err
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'pinnsf', '--nav'])
    assert '--route' in capsys.readouterr().err


def test_scenes_the_field_cannot_route_are_refused_before_any_state():
    """BaseSimulator.simulate_*(nav=) on the CPU: check_nav_scene speaks before scenario_state would ask for a GPU"""
    import torch
    from piml_amd import scenarios
    from piml_amd.models.simulators import BaseSimulator
    from test_simulator_gpu import sim_args
    sim = BaseSimulator(sim_args(device='cpu'))
    sim.model.eval()
    gc = scenarios.gc_scenario()
    assert gc.route_max_iters == 16
    with pytest.raises(ValueError, match='route_max_iters'):
        sim.simulate_scenario(gc, 5, nav=True)
    with pytest.raises(ValueError, match='route_max_iters'):
        sim.simulate_ensemble(gc, 5, [0, 1], nav='sight')
    with pytest.raises(ValueError, match='gates'):
        sim.simulate_scenario(scenarios.crosswalk_scenario(), 5, nav=True)
    with pytest.raises(ValueError, match='grouped'):
        sim.simulate_ensemble(dataclasses.replace(gc, route_max_iters=0, spawn_law='clip_groups'), 5, [0], nav=True)
    with pytest.raises(TypeError):
        sim.simulate_scenario(dataclasses.replace(gc, route_max_iters=0), 5, nav='field')
    with pytest.raises(TypeError):
        sim.simulate_scenario(dataclasses.replace(gc, route_max_iters=0), 5, nav=1.0)
    assert torch.is_grad_enabled()                               # the refusals left the scenario mode
