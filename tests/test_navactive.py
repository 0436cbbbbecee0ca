"""CPU: the floor-field solve by active tiles.  Its numpy restatement (navactive_ref.py) reaches navcost_ref.solve's fixed point
bit for bit on every case of both test files, with both buffers equal at the end, and on the re-activation case a tile goes
quiet and wakes again; every refusal of piml_nav_relax_active that returns before any HIP call, of the Python operators, of the
run loop's schedule and of the command line, each from values that pass but for one thing; and the gfx950 build of
navactive.hip without scratch or spills."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import navactive_ref as REF
import navcost_ref as COST
from conftest import REPO
from test_navfield import PLAN

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. the restatement ----

@pytest.mark.parametrize('name', REF.CASES)
@pytest.mark.parametrize('gates', (False, True))
def test_active_tiles_reach_the_dense_fixed_point(name, gates):
    blocked, goal, c3, c4 = REF.case(name)
    cost = c4 if gates else c3
    r = REF.solved(name, gates)
    u, steps = REF.dense(blocked, goal, cost)
    assert np.array_equal(bits(r.u), bits(u))
    assert np.array_equal(bits(r.u), bits(r.other))          # (so no NaN of the unwritten buffer is left either)
    assert not r.stalled and not r.changed[-1].any()
    # the launch that found nothing changed is the first past the slowest plane's last changing step
    assert r.launches == -(-int(steps.max()) // REF.STEPS) + 1
    ty, tx = REF.tiles(*blocked.shape)
    assert r.active[0].all() and r.active.shape == (r.launches, 6, ty, tx)
    assert np.array_equal(r.work, r.active.sum((0, 2, 3)).reshape(3, 2))
    assert (r.work >= ty * tx).all() and (r.work <= r.launches * ty * tx).all()
    print(f'[navactive] {name} gates={gates}: {r.launches} launches, work {r.work.tolist()} of {r.launches * ty * tx} a plane')


def test_partial_runs_are_the_dense_iterates():
    """after exactly n launches the written buffer is 8 n dense steps, whatever was skipped"""
    blocked, goal, c3, _ = REF.case('65x65')
    for n in (2, 4, 7):
        r = REF.relax_active(blocked, goal, c3, launches=n)
        for p in range(6):
            m, g = divmod(p, 2)
            want = COST.steps(COST.nav_ref.start(goal[g:g + 1]), blocked, goal[g:g + 1], c3[m], REF.STEPS * n)[0]
            assert np.array_equal(bits(r.u[m, g]), bits(want)), (n, p)
        assert r.launches == n and r.stalled == bool(r.changed[-1].any())


def test_a_tile_goes_quiet_and_wakes_again():
    blocked, goal, cost = REF.reactivation_case()
    assert blocked.shape == (65, 161) and goal[0, 16, 2] == 1 and goal.sum() == 1
    r = REF.relax_active(blocked, goal, cost[None])
    u, steps = COST.solve(blocked, goal, cost)
    assert np.array_equal(bits(r.u[0]), bits(u)) and np.array_equal(bits(r.u), bits(r.other))
    ty, tx = REF.tiles(65, 161)
    assert (ty, tx) == (3, 6)
    woken = REF.histories(r.active[:, 0])
    assert woken, 'no tile was active, quiet and active again'
    work, dense_work = int(r.work.sum()), r.launches * ty * tx
    assert r.launches == -(-steps // REF.STEPS) + 1 and ty * tx < work < dense_work
    a = r.active[:, 0, 0, 5]
    print(f'\n[navactive] re-activation: {r.launches} launches, {work} of {dense_work} tile-launches, fixed point after {steps} '
          f'steps; woken tiles (y, x) {woken}; tile (x 5, y 0): ' + ''.join('X' if x else '.' for x in a))
    # too few launches are seen: the last launch still changed a tile
    assert REF.relax_active(blocked, goal, cost[None], launches=2).stalled


# ---- 2. the entry's checks ----

def test_nav_relax_active_refuses_bad_arguments_without_gpu():
    """every refusal comes before any launch, so it needs no GPU; the values that pass are run in test_navactive_gpu.py"""
    from piml_amd import _lib
    L = _lib.lib()
    buf, other = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    a, b = ctypes.addressof(buf), ctypes.addressof(other)

    def call(blocked=a, goal=a, cost=a, per_gate=0, u_a=a, u_b=b, members=1, G=1, gx=2, gy=2, launches=2, flags=a, work=a,
             stalled=a):
        return L.piml_nav_relax_active(blocked, goal, cost, per_gate, u_a, u_b, members, G, gx, gy, launches, flags, work,
                                       stalled, None)
    for kw in (dict(blocked=None), dict(goal=None), dict(cost=None), dict(u_a=None), dict(u_b=None), dict(u_b=a),
               dict(flags=None), dict(stalled=None), dict(members=0), dict(members=-2), dict(G=0), dict(G=65), dict(gx=0),
               dict(gx=1025), dict(gy=0), dict(gy=1025), dict(launches=0), dict(launches=1), dict(launches=3), dict(launches=-2),
               dict(per_gate=2), dict(per_gate=-1), dict(members=1024, G=64),              # 65536 planes
               dict(members=2048, G=1, gx=1024, gy=1024),                                  # 2^31 cells
               dict(members=33, G=64, gx=1024, gy=1024)):
        assert call(**kw) == 1, kw


def test_header_declares_and_lib_binds_the_entry():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    m = re.search(r'\bint piml_nav_relax_active\s*\(([^;]*)\)\s*;', text)
    assert m and hasattr(_lib.lib(), 'piml_nav_relax_active')
    assert len(_lib.SIGNATURES['piml_nav_relax_active']) == 15 == len(m.group(1).split(','))
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols were only added


# ---- 3. build ----

def test_navactive_kernel_builds_for_gfx950_without_scratch_or_spills(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'navactive.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'navactive.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    names = re.findall(r'Function Name: (\S+)', p.stderr)
    assert len(names) == 1 and 'nav_relax_active_kernel' in names[0], names
    for key in (r'ScratchSize \[bytes/lane\]', 'SGPRs Spill', 'VGPRs Spill'):
        assert [int(x) for x in re.findall(key + r': (\d+)', p.stderr)] == [0], key
    lds = int(re.search(r'LDS Size \[bytes/block\]: (\d+)', p.stderr).group(1))
    vgprs = int(re.search(r' VGPRs: (\d+)', p.stderr).group(1))
    print(f'[navactive] nav_relax_active_kernel: {vgprs} VGPRs, {lds} bytes of LDS')
    # nav_relax_cost_kernel's three planes and mask, and the block-wide OR's words; five workgroups still fit a CU's 160 KB
    assert 3 * 48 * 48 * 4 + 48 * 48 <= lds <= 160 * 1024 // 5


# ---- 4. Python checks ----

def test_density_law_takes_a_solver():
    from piml_amd import ops_scenario
    law = ops_scenario.nav_density_law(2.0)
    assert (law.solver, law.max_launches) == ('batch', None)
    assert repr(law) == 'nav_density_law(kd=2.0, rho0=0.5, radius=0.75, fmax=8.0, every=8)'          # today's string
    assert repr(ops_scenario.NavDensityLaw(2.0, 0.5, 0.75, 8.0, 8)) == repr(law)                      # and today's construction
    law = ops_scenario.nav_density_law(2.0, every=2, solver='active')
    assert (law.solver, law.max_launches, law.every) == ('active', None, 2) and "solver='active'" in repr(law)
    law = ops_scenario.nav_density_law(2.0, solver='active', max_launches=40)
    assert law.max_launches == 40 and 'max_launches=40' in repr(law)
    for bad in (dict(solver='dense'), dict(solver=None), dict(solver='Active'), dict(solver=1)):
        with pytest.raises(ValueError, match='solver'):
            ops_scenario.nav_density_law(2.0, **bad)
    with pytest.raises(ValueError, match="solver='active'"):
        ops_scenario.nav_density_law(2.0, max_launches=40)                   # the batch solver has no such bound
    for n in (0, 1, 3, -2, 2.5, True):
        with pytest.raises(ValueError, match='max_launches'):
            ops_scenario.nav_density_law(2.0, solver='active', max_launches=n)


def test_operator_refuses_what_it_cannot_take():
    import torch
    from piml_amd import _lib, ops_scenario
    z8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    for n in (0, 1, 3, -2, 2.5, True):
        with pytest.raises(ValueError, match='launches'):
            ops_scenario.nav_relax_active(z8(3, 3), z8(2, 3, 3), torch.ones(1, 3, 3), n)
    with pytest.raises(_lib.PimlHipError):                                   # everything right but the device
        ops_scenario.nav_relax_active(z8(3, 3), z8(2, 3, 3), torch.ones(1, 3, 3), 2)
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_relax_active(z8(3, 3), z8(2, 3, 3), torch.ones(1, 2, 3, 3), 2)
    with pytest.raises(ValueError, match='blocked'):
        ops_scenario.nav_relax_active(z8(3, 3), z8(2, 3, 4), torch.ones(1, 3, 3), 2)
    with pytest.raises(ValueError, match='blocked'):
        ops_scenario.nav_relax_active(torch.zeros(3, 3), z8(2, 3, 3), torch.ones(1, 3, 3), 2)


def _stand_in(T=40):
    from piml_amd import ops_scenario
    nav = ops_scenario.NavFieldDynamic.__new__(ops_scenario.NavFieldDynamic)
    return type('S', (), dict(T=T))(), nav


def test_schedule_refusals_come_before_any_launch():
    """a captured run takes an every that is a multiple of frames_per_graph or, under solver='active', one that divides it;
    the check needs no GPU: a stand-in field of the right class is enough"""
    from piml_amd import ops_scenario
    from piml_amd.models.mlapm import MLAPM
    st, nav = _stand_in()
    for every, per in ((3, 8), (6, 8), (12, 8), (5, 4)):
        for solver in ('batch', 'active'):
            law = ops_scenario.nav_density_law(2.0, every=every, solver=solver)
            with pytest.raises(ValueError, match='multiple of frames_per_graph'):
                MLAPM._run_scenario(st, None, True, per, nav=nav, nav_density=law)
    for every in (1, 2, 4):                                  # divisors of 8 stay refused under the batch solver
        with pytest.raises(ValueError, match='multiple of frames_per_graph'):
            MLAPM._run_scenario(st, None, True, 8, nav=nav, nav_density=ops_scenario.nav_density_law(2.0, every=every))
    with pytest.raises(ValueError, match='divisor'):         # the active solver's message names both allowed cases
        MLAPM._run_scenario(st, None, True, 8, nav=nav, nav_density=ops_scenario.nav_density_law(2.0, every=3, solver='active'))
    with pytest.raises(TypeError, match='NavFieldDynamic'):
        MLAPM._run_scenario(st, None, True, 8, nav=None, nav_density=ops_scenario.nav_density_law(2.0, every=2, solver='active'))


def test_check_converged_reads_the_stalled_word():
    import torch
    from piml_amd import ops_scenario
    _, nav = _stand_in()
    nav.stalled, nav.max_launches, nav.gx, nav.gy = torch.zeros(1, dtype=torch.int32), 12, 161, 65
    nav.check_converged()
    nav.stalled[0] = 1
    with pytest.raises(RuntimeError, match='max_launches = 12'):
        nav.check_converged()
    nav.base = type('B', (), dict(iterations=384))()
    assert nav.default_max_launches() == 96                  # twice the 48 launches of 8 steps
    nav.base.iterations = 8 * 3
    assert nav.default_max_launches() == 6
    nav.base.iterations = 20                                 # (not a whole number of launches: rounded up, then to even)
    assert nav.default_max_launches() == 6


def test_command_line(tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, n_initial=4)))
    head = ['--law', 'mlapm', '--scene-plan', str(path)]
    dens = head + ['--nav', '--nav-density', '2']
    own, _ = simulate.get_args(dens)
    assert (own.density_law.solver, own.density_law.max_launches) == ('batch', None)
    own, _ = simulate.get_args(dens + ['--nav-solver', 'batch'])
    assert (own.density_law.solver, own.density_law.max_launches) == ('batch', None)
    own, _ = simulate.get_args(dens + ['--nav-solver', 'active', '--nav-every', '2'])
    assert (own.density_law.solver, own.density_law.max_launches, own.density_law.every) == ('active', None, 2)
    own, _ = simulate.get_args(dens + ['--nav-solver', 'active', '--nav-max-launches', '40', '--nav-flow', '1'])
    assert (own.density_law.solver, own.density_law.max_launches, own.density_law.flow) == ('active', 40, 1.0)
    for argv in (head + ['--nav', '--nav-solver', 'active'], head + ['--nav', '--nav-max-launches', '40'],
                 head + ['--nav-solver', 'active'], dens + ['--nav-solver', 'dense'], dens + ['--nav-max-launches', '40'],
                 dens + ['--nav-solver', 'batch', '--nav-max-launches', '40'],
                 dens + ['--nav-solver', 'active', '--nav-max-launches', '41'],
                 dens + ['--nav-solver', 'active', '--nav-max-launches', '0'],
                 dens + ['--nav-solver', 'active', '--nav-max-launches', '2.5'],
                 head + ['--nav', '--nav-sight', '--nav-density', '2', '--nav-solver', 'active'],
                 ['--checkpoint', 'm.pt', '--scene-plan', str(path), '--route', 'field', '--nav-density', '2', '--nav-solver',
                  'active']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)
