"""CPU: the fluctuation term of the MLAPM scenario frame without a GPU -- the numpy restatement's draws (moments of 131 072
normals) and its Ornstein-Uhlenbeck recursion (stationary variance, lag-1 autocorrelation), noise_law / noise_args / sweep_noise
and their refusals, the argument checks of piml_scenario_step_mlapm_noise and piml_noise_force through the library (no
launch), and simulate's JSON reader."""
import ctypes
import json
import math

import numpy as np
import pytest

import noise_ref as R
from test_abi import declared_symbols
from test_scenario_groups import _descriptor

INVALID = 1
SEEDS, FRAMES, SLOTS = range(8), 256, 32
PLAIN = dict(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)


def all_draws():
    """z (8 seeds, 256 frames, 32 slots, 2)"""
    return np.stack([np.stack([R.draws(s, t, np.arange(SLOTS)) for t in range(FRAMES)]) for s in SEEDS])


Z = None


def z_all():
    global Z
    if Z is None:
        Z = all_draws()
    return Z


def test_moments_of_the_draws():
    z = z_all().astype(np.float64).reshape(-1)
    n = z.size
    assert n == 131072
    mean, var, top = z.mean(), z.var(), np.abs(z).max()
    print(f'\n[noise] {n} normals: |mean| {abs(mean):.2e} (bound {4 / math.sqrt(n):.4f}), |var - 1| {abs(var - 1):.4f} '
          f'(bound {4 * math.sqrt(2 / n):.4f}), max |z| {top:.2f}')
    assert abs(mean) <= 4 / math.sqrt(n)                      # four standard errors
    assert abs(var - 1) <= 4 * math.sqrt(2 / n)
    assert top <= math.sqrt(48 * math.log(2)) + 1e-6          # u1 >= 2^-24
    # the two components and two seeds are different streams; a frame >= 2^32 reaches the counter's second word
    zz = z_all()
    assert not np.array_equal(zz[..., 0], zz[..., 1]) and not np.array_equal(zz[0], zz[1])
    assert not np.array_equal(R.draws(3, 5, np.arange(4)), R.draws(3, 5 + (1 << 32), np.arange(4)))
    assert not np.array_equal(R.draws(4, 5, np.arange(4)), R.draws((1 << 63) + 4, 5, np.arange(4)))


def test_ou_recursion_is_stationary_with_the_laws_constants():
    dt, tau, An = 0.08, 0.5, 0.4
    rho, amp = R.law(An, tau, dt)
    assert rho == np.float32(0.85214376) and amp == np.float32(0.20932308)
    z = z_all()                                               # (seed, frame, slot, 2): one chain per (seed, slot, component)
    eta = np.zeros(z[:, 0].shape, np.float32)
    chain = []
    for t in range(FRAMES):
        eta = R.step(eta, rho, amp, z[:, t])
        chain.append(eta)
    x = np.stack(chain)[64:].astype(np.float64)               # frames 64 .. 255: 64 frames are 10 correlation times
    n = x.size
    r = float(rho)
    n_eff = n * (1 - r * r) / (1 + r * r)
    var = (x * x).mean()
    ac1 = (x[1:] * x[:-1]).mean() / var
    print(f'\n[noise] OU: var / An^2 - 1 = {var / An ** 2 - 1:.2e} (bound {4 * math.sqrt(2 / n_eff):.3f}), lag-1 autocorrelation '
          f'{ac1:.4f} (rho {r:.4f})')
    assert 4 * math.sqrt(2 / n_eff) == pytest.approx(0.045, abs=5e-4)
    assert abs(var / An ** 2 - 1) <= 4 * math.sqrt(2 / n_eff)
    assert abs(ac1 - r) <= 0.02
    # white noise: eta = An z exactly, whatever eta was
    rho0, amp0 = R.law(An, 0.0, dt)
    assert rho0 == 0 and amp0 == np.float32(An)
    assert np.array_equal(R.step(chain[-1], rho0, amp0, z[:, 0]), (np.float32(An) * z[:, 0]).astype(np.float32))
    # present == 0 rows keep their eta and draw nothing
    e0 = chain[3][:2]
    present = np.zeros((2, SLOTS), np.uint8)
    present[0, ::2] = 1
    out, zz = R.force(e0, [0, 1], 4, rho, amp, present)
    assert np.array_equal(out[1], e0[1]) and (zz[1] == 0).all() and np.array_equal(out[0, 1::2], e0[0, 1::2])
    assert np.array_equal(out[0, ::2], chain[4][0, ::2])


def test_noise_law_and_its_refusals():
    from piml_amd import _lib, ops_scenario
    law = ops_scenario.noise_law(0.4, 0.5, 0.08)
    assert isinstance(law, _lib.NoiseLaw) and (np.float32(law.rho), np.float32(law.amp)) == R.law(0.4, 0.5, 0.08)
    white = ops_scenario.noise_law(0.4, 0.0, 0.08)
    assert white.rho == 0.0 and np.float32(white.amp) == np.float32(0.4)
    assert ops_scenario.noise_law(0.4, 0.0, 0.01).amp == white.amp            # white noise: An per frame whatever dt is
    zero = ops_scenario.noise_law(0.0, 0.5, 0.08)
    assert zero.amp == 0.0 and zero.rho > 0
    nan, inf = float('nan'), float('inf')
    for An, tau, dt in ((-0.1, 0.5, 0.08), (nan, 0.5, 0.08), (inf, 0.5, 0.08), (0.4, -0.5, 0.08), (0.4, nan, 0.08),
                        (0.4, inf, 0.08), (0.4, 0.5, 0.0), (0.4, 0.5, -0.08), (0.4, 0.5, nan), (0.4, 0.5, inf),
                        (0.4, 1e12, 0.08)):                   # (rho would round to 1)
        with pytest.raises(ValueError):
            ops_scenario.noise_law(An, tau, dt)
    with pytest.raises(ValueError):
        ops_scenario.noise_law_table([], 0.08)
    with pytest.raises(ValueError):
        ops_scenario.noise_law_table([(0.4, -1.0)], 0.08)
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.noise_law_table([(0.4, 0.5)], 0.08, device='cpu')
    import torch
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.noise_force(torch.zeros(4, 2), 0, 0, 0.4, 0.5, 0.08)     # no CPU path
    assert ctypes.sizeof(_lib.NoiseLaw) == 8 and ctypes.sizeof(_lib.NoiseArgs) == 24


def test_model_arguments():
    from piml_amd.models import mlapm as M
    assert M.NOISE_KEYS == ('An', 'noise_tau')
    assert M.noise_args(dict(PLAIN)) is None
    assert M.noise_args(dict(PLAIN, An=0.5)) == (0.5, 0.0) and M.noise_args(dict(An=0.5, noise_tau=0.3)) == (0.5, 0.3)
    for bad in (dict(noise_tau=0.3), dict(An=-1.0), dict(An=float('nan')), dict(An=0.5, noise_tau=-0.1),
                dict(An=0.5, noise_tau=float('inf'))):
        with pytest.raises(ValueError):
            M.noise_args(bad)
        with pytest.raises(ValueError):
            M.MLAPM(**PLAIN, **bad)
    assert M.MLAPM(**PLAIN, An=0.5).args['An'] == 0.5
    # sweeps: any subset of the candidates may carry the term
    assert M.sweep_noise([dict(PLAIN), dict(PLAIN)]) is None
    assert M.sweep_noise([dict(PLAIN, An=0.5, noise_tau=0.3), dict(PLAIN), dict(PLAIN, An=0.0)]) == [(0.5, 0.3), (0.0, 0.0), (0.0, 0.0)]
    assert len(M.sweep_laws([dict(PLAIN, An=0.5, noise_tau=0.3), dict(PLAIN)])) == 2
    with pytest.raises(ValueError):
        M.sweep_laws([dict(PLAIN, noise_tau=0.3)])
    with pytest.raises(ValueError):
        M.sweep_laws([dict(PLAIN, An=0.5, noise=1.0)])


def test_symbols_and_structs():
    from piml_amd import _lib
    names = {'piml_noise_force', 'piml_scenario_step_mlapm_noise'}
    assert names <= set(declared_symbols(('piml_hip.h',))) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.piml_abi_version() == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES['piml_noise_force']) == 11 and len(_lib.SIGNATURES['piml_scenario_step_mlapm_noise']) == 16


def test_entry_checks_return_before_any_launch():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    seeds = (ctypes.c_uint64 * 2)(0, 1)
    law = ops_scenario.mlapm_law()
    wall = ops_scenario.wall_law(50.0, -5.0)

    def noise(rho=0.85, amp=0.2, state=0x1000, table=None):
        na = _lib.NoiseArgs()
        na.state, na.law.rho, na.law.amp, na.law_table = state, rho, amp, table
        return na

    def call(s, r, g, na, members=2, sd=seeds, law=law, table=None, grid=None, wall=None, wtable=None, glaw=None, gtable=None,
             init=0, offset=0):
        ref = lambda x: None if x is None else (x if isinstance(x, int) else ctypes.byref(x))
        return L.piml_scenario_step_mlapm_noise(ref(s), ref(r), members, sd, ref(law), table, ref(grid), ref(wall), wtable,
                                                ref(g), ref(glaw), gtable, ref(na), init, offset, None)
    nan, inf = float('nan'), float('inf')
    for grouped in (True, False):
        s, r, g = _descriptor() if grouped else _descriptor(6)
        if not grouped:
            g = None
        # the noise arguments
        assert call(s, r, g, None) == INVALID and call(s, r, g, noise(state=None)) == INVALID
        for rho, amp in ((nan, 0.2), (inf, 0.2), (-0.1, 0.2), (1.0, 0.2), (1.5, 0.2), (0.85, nan), (0.85, inf), (0.85, -0.2)):
            assert call(s, r, g, noise(rho, amp)) == INVALID, (rho, amp)
            assert call(s, r, g, noise(rho, amp), init=1) == INVALID, (rho, amp)
        # what the frame entries check
        ok = noise()
        assert call(None, r, g, ok) == call(s, r, g, ok, sd=None) == INVALID
        assert call(s, r, g, ok, members=0) == call(s, r, g, ok, members=65536) == call(s, r, g, ok, offset=-1) == INVALID
        assert call(s, r, g, ok, init=2) == call(s, r, g, ok, init=-1) == INVALID
        for field, value in (('P', 4), ('capacity', 0), ('entries', None), ('n_initial', 6), ('spawn_cap', 9),
                             ('position_out', None), ('D', 9)):
            s2 = _descriptor()[0]
            setattr(s2, field, value)
            assert call(s2, r, g, ok) == INVALID, field
        assert call(s, r, g, ok, law=None) == call(s, r, g, ok, table=0x1000) == INVALID          # exactly one law form
        bad_law = ops_scenario.mlapm_law()
        bad_law.tau = 0.0
        assert call(s, r, g, ok, law=bad_law) == INVALID
        assert call(s, r, g, ok, wall=wall) == call(s, r, g, ok, wtable=0x1000) == INVALID        # a wall law without a grid
        assert call(s, r, g, ok, grid=_lib.WallGrid(), wall=wall) == INVALID                      # an all-zero grid
        grid = ops_scenario.wall_grid_desc(ops_scenario.wall_grid_host(np.array([[0.0, 0.0], [1.0, 1.0]], np.float32)), 0x1000,
                                           0x1000)
        assert call(s, r, g, ok, grid=grid) == call(s, r, g, ok, grid=grid, wall=wall, wtable=0x1000) == INVALID
    # a grouped scene: the group checks; an ungrouped one: no group law, no init launch, not the grouped spawn law
    s, r, g = _descriptor()
    ok = noise()
    glaw = ops_scenario.group_law(3.0, 0.5)
    assert call(s, _descriptor(6)[1], g, ok) == INVALID and call(s, None, g, ok) == INVALID
    g2 = _descriptor()[2]
    g2.group_first = None
    assert call(s, r, g2, ok) == INVALID
    bad = _lib.GroupLaw()
    bad.A, bad.dist = -1.0, 0.5
    assert call(s, r, g, ok, glaw=bad) == call(s, r, g, ok, glaw=glaw, gtable=0x1000) == INVALID
    s, r, _ = _descriptor(6)
    assert call(s, r, None, ok, glaw=glaw) == call(s, r, None, ok, gtable=0x1000) == call(s, r, None, ok, init=1) == INVALID
    assert call(s, _descriptor()[1], None, ok) == INVALID      # PIML_SPAWN_CLIP_GROUPS without its groups
    # piml_noise_force
    f = L.piml_noise_force
    assert f(0x1000, None, 0x1000, None, seeds, -1, 4, 0, 0.85, 0.2, None) == INVALID
    assert f(0x1000, None, 0x1000, None, seeds, 2, -4, 0, 0.85, 0.2, None) == INVALID
    assert f(0x1000, None, 0x1000, None, seeds, 2, 4, -1, 0.85, 0.2, None) == INVALID
    for rho, amp in ((nan, 0.2), (-0.1, 0.2), (1.0, 0.2), (0.85, inf), (0.85, -0.2)):
        assert f(0x1000, None, 0x1000, None, seeds, 2, 4, 0, rho, amp, None) == INVALID
    assert f(None, None, 0x1000, None, seeds, 2, 4, 0, 0.85, 0.2, None) == INVALID
    assert f(0x1000, None, None, None, seeds, 2, 4, 0, 0.85, 0.2, None) == INVALID
    assert f(0x1000, None, 0x1000, None, None, 2, 4, 0, 0.85, 0.2, None) == INVALID
    assert f(None, None, None, None, None, 0, 4, 0, 0.85, 0.2, None) == 0      # nothing to do, nothing launched
    assert f(None, None, None, None, None, 2, 0, 0, 0.0, 0.0, None) == 0


def test_simulates_json_reader_accepts_the_two_keys(tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'law.json'
    path.write_text(json.dumps(dict(PLAIN, An=0.5, noise_tau=0.3)))
    got = simulate.load_mlapm_params(str(path))
    assert got['An'] == 0.5 and got['noise_tau'] == 0.3 and got['A'] == 7.55
    path.write_text(json.dumps(dict(PLAIN, An=0.5)))
    assert 'noise_tau' not in simulate.load_mlapm_params(str(path))
    for bad in (dict(noise_tau=0.3), dict(An=-0.5), dict(An='0.5'), dict(An=True), dict(An=0.5, noise_tau=-1)):
        path.write_text(json.dumps(dict(PLAIN, **bad)))
        with pytest.raises(ValueError):
            simulate.load_mlapm_params(str(path))
