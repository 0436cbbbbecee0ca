"""CPU: the direction-aware density's numpy restatement (navflow_ref.py) -- on the two-room, two-door plan a queue walking
towards gate 0 opens its door to gate 0's walkers and closes it to gate 1's, the same queue walking the other way does the
opposite, a standing one is the head count, and flow = 0 is navcost_ref.cost bit for bit whatever the velocities --, the
descent direction's properties, the argument checks of piml_nav_descent, piml_nav_flow, piml_nav_cost_flow and
piml_nav_relax_cost_gates that return before any HIP call, the Python and command-line refusals, and the gfx950 build of
navflow.hip without scratch or spills."""
import ctypes
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref
import navcost_ref as COST
import navflow_ref as REF
from conftest import REPO
from test_navfield import BASE, PLAN

f32 = np.float32
NAN, INF = float('nan'), float('inf')
PROTO = dict(cell=COST.TWO_DOOR_CELL, r=1, kd=2.0, rho0=0.5, fmax=8.0, vref=1.3)
# (flow, the queue's velocity) -> per gate, whether each probe reaches the wall's column in the NEAR door
HEADS0, HEADS1 = [False, False, False, False, False, True, False], [False, False, False, False, False, True, False]
FLOWING = [True] * 7
PROTO_ROWS = (((0.0, (1.3, 0.0)), (HEADS0, HEADS1)),
              ((1.0, (1.3, 0.0)), (FLOWING, [False] * 7)),
              ((1.0, (-1.3, 0.0)), (HEADS0, FLOWING)),
              ((1.0, (0.0, 0.0)), (HEADS0, HEADS1)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def proto_planes(flow, vel):
    """the prototype's cost planes (2, gy, gx) for the queue of 25 all walking at `vel`"""
    blocked, goal, count = REF.two_door_two_gates()
    d = REF.descent_dir(nav_ref.solve(blocked, goal)[0])
    P = COST.two_door_positions()[None]
    V = np.tile(np.array(vel, f32), (1, 25, 1))
    cnt, mom = REF.deposit_flow(P, V, np.ones((1, 25), f32), 0.0, 0.0, PROTO['cell'], 40, 24)
    assert np.array_equal(cnt[0], count)
    f = REF.cost_flow(cnt, mom, d, PROTO['cell'], PROTO['r'], PROTO['kd'], PROTO['rho0'], PROTO['fmax'], flow, PROTO['vref'])
    return blocked, goal, count, f[0]


# ---- 1. the restatement ----

def test_two_doors_a_stream_towards_my_gate_opens_its_door():
    """Rows reached on the wall's column by navcost_ref.descend (near door = rows 4..6, far door = rows 17..19):

        flow  queue velocity  gate 0                  gate 1
        0     (+1.3, 0)       17 17 17 17 17 5 17     17 17 17 17 17 6 17
        1     (+1.3, 0)       6 6 6 6 6 5 5           17 17 17 17 17 17 17
        1     (-1.3, 0)       as flow = 0             6 6 6 6 6 5 5
        1     (0, 0)          as flow = 0             as flow = 0

    Steps of the solve per gate, as first seen (not asserted): 63 / 63; 58 / 63; 63 / 56; 63 / 63."""
    for (flow, vel), want in PROTO_ROWS:
        blocked, goal, count, f = proto_planes(flow, vel)
        assert f.min() >= 1.0 and f.max() <= 8.0
        u, steps = REF.solve_gates(blocked, goal, f)
        for g, probes in enumerate((COST.TWO_DOOR_PROBES, REF.GATE1_PROBES)):
            rows = [COST.descend(u[g], x, y, COST.TWO_DOOR_WALL) for x, y in probes]
            print(f'[navflow] flow {flow} v {vel} gate {g}: rows {rows}, {steps[g]} steps')
            assert all(r in COST.NEAR_DOOR + COST.FAR_DOOR for r in rows), (flow, vel, g, rows)
            assert [r in COST.NEAR_DOOR for r in rows] == want[g], (flow, vel, g, rows)
        scalar, _ = COST.cost(count, PROTO['cell'], PROTO['r'], PROTO['kd'], PROTO['rho0'], PROTO['fmax'])
        same = [np.array_equal(bits(f[g]), bits(scalar)) for g in range(2)]
        assert same == ([True, True] if flow == 0.0 or vel == (0.0, 0.0) else [False, False])


def test_flow_zero_is_the_scalar_cost_bit_for_bit_whatever_the_velocities():
    blocked, goal = nav_ref.u_shape_case()
    gy, gx = blocked.shape
    rng = np.random.default_rng(5)
    d = REF.descent_dir(nav_ref.solve(blocked, goal)[0])
    P = rng.uniform(-1.0, 18.0, (3, 400, 2)).astype(f32)         # cells of 0.5 from (0, 0): some fall outside
    V = rng.normal(0, 2.0, (3, 400, 2)).astype(f32)
    V[:, 0], V[:, 1], V[:, 2], V[:, 3], V[:, 4] = (NAN, 1.0), (INF, -INF), (20.0, -20.0), (-20.0, NAN), (0.0, 1e30)
    mask = (rng.uniform(size=(3, 400)) < 0.9).astype(f32)
    mask[:, :5] = 1
    P[:, :5, 0], P[:, :5, 1] = 1.1 + np.arange(5, dtype=f32), 1.2          # the special velocities are counted, a cell each
    cnt, mom = REF.deposit_flow(P, V, mask, 0.0, 0.0, 0.5, gx, gy)
    assert np.abs(mom).max() > 4096 and cnt.sum() > 600
    for r in (0, 1, 3):
        scalar, _ = COST.cost(cnt, 0.5, r, 2.0, 0.5, 8.0)
        f = REF.cost_flow(cnt, mom, d, 0.5, r, 2.0, 0.5, 8.0, 0.0, 1.3)
        assert f.shape == (3, 2, gy, gx) and (scalar > 1).any()
        for g in range(2):
            assert np.array_equal(bits(f[:, g]), bits(scalar)), (r, g)
        moved = REF.cost_flow(cnt, mom, d, 0.5, r, 2.0, 0.5, 8.0, 1.0, 1.3)
        assert not np.array_equal(bits(moved[:, 0]), bits(scalar)) and not np.array_equal(bits(moved[:, 0]), bits(moved[:, 1]))
        assert moved.min() >= 1.0 and moved.max() <= 8.0         # f >= 1 also where s_eff < 0


def test_the_deposit_quantises_as_stated():
    q = REF.quantise(np.array([0.0, 1.3, -1.3, 20.0, -20.0, 8.0, NAN, INF, -INF, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024], f32))
    assert q.tolist() == [0, 1331, -1331, 8192, -8192, 8192, 0, 0, 0, 0, 2, 2, 0]       # halves to even; not finite is 0
    P = np.array([[[0.1, 0.1], [0.1, 0.1], [0.6, 0.1], [NAN, 0.1], [5.0, 0.1], [0.1, 0.1]]], f32)
    V = np.array([[[1.0, -1.0], [0.5, 2.0], [NAN, 3.0], [1.0, 1.0], [1.0, 1.0], [7.0, 7.0]]], f32)
    cnt, mom = REF.deposit_flow(P, V, np.array([[1, 1, 1, 1, 1, 0]], f32), 0.0, 0.0, 0.5, 2, 1)
    assert cnt.tolist() == [[[2, 1]]]                            # NaN position, outside and absent: no count, no momentum
    assert mom.tolist() == [[[[1536, 0]], [[1024, 3072]]]]


def test_descent_dir_on_the_u_shape():
    blocked, goal = nav_ref.u_shape_case()
    u, _ = nav_ref.solve(blocked, goal)
    d = REF.descent_dir(u)
    assert d.shape == (2, 34, 33, 2) and d.dtype == f32
    n = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
    for g in range(2):
        zero = (goal[g] != 0) | ~np.isfinite(u[g])
        assert (d[g][zero] == 0).all() and not np.isfinite(u[g][20, 30]) and (d[g, 20, 30] == 0).all()      # the enclosed cell
        assert (d[g][(blocked != 0) & (goal[g] == 0)] == 0).all()
        assert np.abs(n[g][~zero] - 1.0).max() <= 2 * np.finfo(f32).eps and (~zero).sum() > 900           # unit within 2 ulp
    assert goal[1, 5, 8] and blocked[5, 8] and (d[1, 5, 8] == 0).all()       # a goal on a blocked cell behaves as a goal ...
    assert u[1, 5, 8] == 0 and d[1, 4, 8, 1] > 0                             # ... and the cell below it descends up to it
    assert d[0, 5, 8, 0] == 0 and d[0, 5, 8, 1] == 0                         # for gate 0 the same cell is a wall
    # open space inside the U, a clear line to gate 0 at (x 17, y 8): within 45 degrees of the gate
    ys, xs = np.mgrid[6:30, 9:26]
    to = np.stack([17 - xs, 8 - ys], -1).astype(np.float64)
    far = np.hypot(to[..., 0], to[..., 1]) > 0
    cos = (d[0, 6:30, 9:26].astype(np.float64) * to).sum(-1)[far] / np.hypot(to[..., 0], to[..., 1])[far]
    assert cos.min() >= np.cos(np.pi / 4) - 1e-6
    flat = REF.descent_dir(np.full((1, 3, 3), 2.0, f32))         # a plateau: no neighbour is lower
    assert (flat == 0).all()
    tie = REF.descent_dir(np.array([[[1.0, 2.0, 1.0]]], f32))    # L == R: the tie goes to +x
    assert tie[0, 0, 1].tolist() == [1.0, 0.0]


# ---- 2. the entries' refusals, without a device ----

def _bufs():
    buf, other = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    return buf, other, ctypes.addressof(buf), ctypes.addressof(other)


def test_nav_descent_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(u=a, G=1, gx=2, gy=2, d=b):
        return L.piml_nav_descent(u, G, gx, gy, d, None)
    for kw in (dict(u=None), dict(d=None), dict(G=0), dict(G=65), dict(G=-1), dict(gx=0), dict(gx=1025), dict(gy=0), dict(gy=1025)):
        assert call(**kw) == 1, kw


def test_nav_flow_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(pos=a, vel=a, mask=a, members=1, cap=4, x0=0.0, y0=0.0, cell=0.5, gx=2, gy=2, count=b, mom=b):
        return L.piml_nav_flow(pos, vel, mask, members, cap, x0, y0, cell, gx, gy, count, mom, None)
    for kw in (dict(pos=None), dict(vel=None), dict(mask=None), dict(count=None), dict(mom=None), dict(members=0),
               dict(members=65536), dict(cap=0), dict(cap=-1), dict(cap=1 << 18), dict(cap=1 << 30), dict(gx=0), dict(gx=1025),
               dict(gy=0), dict(gy=1025), dict(cell=0.0), dict(cell=-1.0), dict(cell=NAN), dict(cell=INF), dict(x0=NAN),
               dict(x0=INF), dict(y0=-INF), dict(y0=NAN)):
        assert call(**kw) == 1, kw


def test_nav_cost_flow_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(count=a, mom=a, d=a, members=1, G=1, gx=2, gy=2, cell=0.5, r=1, kd=2.0, rho0=0.5, fmax=8.0, flow=1.0, vref=1.3, cost=b):
        return L.piml_nav_cost_flow(count, mom, d, members, G, gx, gy, cell, r, kd, rho0, fmax, flow, vref, cost, None)
    for kw in (dict(count=None), dict(mom=None), dict(d=None), dict(cost=None), dict(members=0), dict(members=65536), dict(G=0),
               dict(G=65), dict(members=1024, G=64), dict(members=33, G=64, gx=1024, gy=1024), dict(gx=0), dict(gx=1025),
               dict(gy=0), dict(gy=1025), dict(cell=0.0), dict(cell=NAN), dict(cell=INF), dict(r=-1), dict(r=9), dict(kd=-0.5),
               dict(kd=NAN), dict(kd=INF), dict(rho0=-0.1), dict(rho0=NAN), dict(rho0=INF), dict(fmax=0.5), dict(fmax=NAN),
               dict(fmax=INF), dict(flow=-0.5), dict(flow=NAN), dict(flow=INF), dict(vref=0.0), dict(vref=-1.3), dict(vref=NAN),
               dict(vref=INF)):
        assert call(**kw) == 1, kw


def test_nav_relax_cost_gates_refuses_bad_arguments_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    _keep1, _keep2, a, b = _bufs()

    def call(blocked=a, goal=a, cost=a, u_a=a, u_b=b, members=1, G=1, gx=2, gy=2, launches=0, changed=a):
        return L.piml_nav_relax_cost_gates(blocked, goal, cost, u_a, u_b, members, G, gx, gy, launches, changed, None)
    assert call() == 0 and call(members=1023, G=64, gx=1024, gy=1) == 0          # no launch: these pass every check
    for kw in (dict(blocked=None), dict(goal=None), dict(cost=None), dict(u_a=None), dict(u_b=None), dict(u_b=a),
               dict(changed=None), dict(members=0), dict(members=-2), dict(G=0), dict(G=65), dict(gx=0), dict(gx=1025), dict(gy=0),
               dict(gy=1025), dict(launches=-1), dict(members=1024, G=64),                  # 65536 planes
               dict(members=2048, G=1, gx=1024, gy=1024),                                   # 2^31 cells
               dict(members=33, G=64, gx=1024, gy=1024)):
        assert call(**kw) == 1, kw
    assert call(members=2047, G=1, gx=1024, gy=1024) == 0                                   # 2^31 - 2^20 cells


def test_header_declares_and_lib_binds_the_entries():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'piml_hip.h')).read(), flags=re.S)
    for name, n in (('piml_nav_descent', 6), ('piml_nav_flow', 13), ('piml_nav_cost_flow', 16), ('piml_nav_relax_cost_gates', 12)):
        m = re.search(r'\bint %s\s*\(([^;]*)\)\s*;' % name, text)
        assert m and hasattr(_lib.lib(), name), name
        assert len(_lib.SIGNATURES[name]) == n == len(m.group(1).split(',')), name
    assert _lib.ABI_VERSION == 35 and _lib.lib().piml_abi_version() == 35        # symbols were only added


# ---- 3. build ----

def test_navflow_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'navflow.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'navflow.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    names = re.findall(r'Function Name: (\S+)', p.stderr)
    assert len(names) == 4, names
    for k in ('nav_descent_kernel', 'nav_flow_kernel', 'nav_cost_flow_kernel', 'nav_relax_cost_gates_kernel'):
        assert any(k in n for n in names), names
    for key in (r'ScratchSize \[bytes/lane\]', 'SGPRs Spill', 'VGPRs Spill'):
        got = [int(x) for x in re.findall(key + r': (\d+)', p.stderr)]
        assert got == [0] * 4, (key, dict(zip(names, got)))
    lds = [int(x) for x in re.findall(r'LDS Size \[bytes/block\]: (\d+)', p.stderr)]
    # the cost kernel stages through nav_cost_kernel's two buffers, whatever the number of gates; the solver's LDS is
    # nav_relax_cost_kernel's
    assert lds == [0, 0, 48 * 48 * 4 + 48 * 32 * 4, 3 * 48 * 48 * 4 + 48 * 48]


# ---- 4. Python checks ----

def test_density_law_takes_flow_and_vref():
    from piml_amd import ops_scenario
    law = ops_scenario.nav_density_law(2.0)
    assert (law.flow, law.vref) == (0.0, 1.3)
    assert repr(law) == 'nav_density_law(kd=2.0, rho0=0.5, radius=0.75, fmax=8.0, every=8)'          # today's string
    assert repr(ops_scenario.nav_density_law(2.0, flow=0, vref=2.0)) == repr(law)
    five = ops_scenario.NavDensityLaw(2.0, 0.5, 0.75, 8.0, 8)    # the five-argument construction still works
    assert (five.flow, five.vref) == (0.0, 1.3) and repr(five) == repr(law)
    law = ops_scenario.nav_density_law(2.0, flow=1, vref=1.5)
    assert (law.flow, law.vref) == (1.0, 1.5) and repr(law).endswith('every=8, flow=1.0, vref=1.5)')
    for bad in (dict(flow=-0.1), dict(flow=NAN), dict(flow=INF), dict(vref=0.0), dict(vref=-1.0), dict(vref=NAN), dict(vref=INF)):
        with pytest.raises(ValueError, match='flow'):
            ops_scenario.nav_density_law(2.0, **bad)


def test_operators_refuse_what_they_cannot_take():
    import torch
    from piml_amd import _lib, ops_scenario, scenarios
    from piml_amd.models import mlapm
    from piml_amd.models.simulators import BaseSimulator
    law = ops_scenario.nav_density_law(2.0, flow=1.0)
    for call in (lambda: ops_scenario.nav_descent(None), lambda: ops_scenario.nav_flow(torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4), None),
                 lambda: ops_scenario.nav_cost_flow(None, None, None, None, law),
                 lambda: ops_scenario.NavFieldDynamic(None, 2, flow=True)):
        with pytest.raises(TypeError):
            call()
    z8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.nav_relax_cost_gates(z8(3, 3), z8(2, 3, 3), torch.ones(1, 2, 3, 3))
    with pytest.raises(ValueError):
        ops_scenario.nav_relax_cost_gates(z8(3, 3), z8(2, 3, 4), torch.ones(1, 2, 3, 3))
    # a law with a flow term joins the runs a density term joins, and no others
    gc = dataclasses.replace(scenarios.gc_scenario(), route_max_iters=0)
    sim = mlapm.MLAPM(**BASE)
    with pytest.raises(ValueError, match='needs nav'):
        sim.simulate_scenario(gc, 5, device='cpu', nav_density=law)
    with pytest.raises(ValueError, match='any-angle'):
        sim.simulate_ensemble(gc, 5, [0, 1], device='cpu', nav='sight', nav_density=law)
    with pytest.raises(ValueError, match='needs nav'):
        mlapm.SweepRun(gc, 5, 1, [0], device='cpu', nav_density=law)
    for name in ('simulate_scenario', 'simulate_ensemble'):
        with pytest.raises(NotImplementedError, match='not built'):
            getattr(BaseSimulator, name)(None, gc, 5, [0], nav=True, nav_density=law)


def test_update_needs_a_field_built_for_flow():
    """nav_field_update's checks come before any launch: a stand-in field of the right class is enough"""
    from piml_amd import ops_scenario

    class Seeds:
        def numel(self):
            return 2
    field = ops_scenario.NavFieldDynamic.__new__(ops_scenario.NavFieldDynamic)
    field.members, field.flow = 2, False
    field.u = type('T', (), dict(device='cpu'))()
    st = type('S', (), dict(seeds=Seeds(), p=type('T', (), dict(device='cpu'))()))()
    with pytest.raises(ValueError, match='flow=True'):
        ops_scenario.nav_field_update(field, st, ops_scenario.nav_density_law(2.0, flow=0.5))


def test_command_line(tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'plan.json'
    path.write_text(json.dumps(dict(PLAN, n_initial=4)))
    head = ['--law', 'mlapm', '--scene-plan', str(path)]
    own, _ = simulate.get_args(head + ['--nav', '--nav-density', '2', '--nav-flow', '1'])
    law = own.density_law
    assert (law.kd, law.every, law.flow, law.vref) == (2.0, 8, 1.0, 1.3)
    own, _ = simulate.get_args(head + ['--nav', '--nav-density', '2', '--nav-flow', '0.5', '--nav-vref', '1.5', '--nav-every', '16'])
    law = own.density_law
    assert (law.kd, law.every, law.flow, law.vref) == (2.0, 16, 0.5, 1.5)
    own, _ = simulate.get_args(head + ['--nav', '--nav-density', '2'])
    assert (own.density_law.flow, own.density_law.vref) == (0.0, 1.3)
    for argv in (head + ['--nav', '--nav-flow', '1'], head + ['--nav', '--nav-vref', '1.3'], head + ['--nav-flow', '1'],
                 head + ['--nav', '--nav-density', '2', '--nav-flow', '-1'], head + ['--nav', '--nav-density', '2', '--nav-flow', 'nan'],
                 head + ['--nav', '--nav-density', '2', '--nav-flow', '1', '--nav-vref', '0'],
                 head + ['--nav', '--nav-density', '2', '--nav-vref', 'inf'],
                 head + ['--nav', '--nav-sight', '--nav-density', '2', '--nav-flow', '1'],
                 ['--checkpoint', 'm.pt', '--scene-plan', str(path), '--route', 'field', '--nav-density', '2', '--nav-flow', '1']):
        with pytest.raises(SystemExit):
            simulate.get_args(argv)
