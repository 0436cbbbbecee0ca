"""GPU: the fluctuation term of the MLAPM scenario frame (piml_scenario_step_mlapm_noise, piml_noise_force) on the
hand-made scene of tests/test_scenario_groups_gpu.py -- capacity 20, 12 frames, seeds 4, 11 and 2^63 + 4: one agent per wave
and four per block, so the slots cross blocks; seed 11 passes the capacity; 4 and 2^63 + 4 differ in the key's high word only.
The operator against the numpy restatement (tests/noise_ref.py), the frame against the operators in its four forms, members,
captured replays, sweeps and their reset, runs without the term, and a small fit of An to track statistics."""
import functools

import numpy as np
import pytest
import torch

import noise_ref as R
from conftest import bits as nbits
from test_scenario_groups_gpu import (AG, AW, BW, CAP, CUTOFF, DEV, GDIST, MLAPM, PLAIN, SEEDS, T, at_spawn, same_arrivals,
                                      scene)
from test_scenario_mlapm_gpu import FIELDS, LAW, _same, _step_fwd, bits

pytestmark = pytest.mark.gpu
AN, NTAU = 0.5, 0.3
DT = 0.08
NOISY = dict(PLAIN, An=AN, noise_tau=NTAU)


# ---- 1. the operator ----

def ulp_close(got, want):
    """within one float32 ulp of the restatement's value"""
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


@pytest.mark.parametrize('N', [37, 300])                      # one block with idle threads; 900 rows in four blocks
def test_noise_force_is_the_restatement(N):
    from piml_amd import _lib, ops_scenario
    rng = np.random.default_rng(N)
    eta = rng.standard_normal((len(SEEDS), N, 2)).astype(np.float32)
    present = (rng.random((len(SEEDS), N)) < 0.7)
    present[:, 0], present[:, -1] = True, False
    dev = torch.tensor(eta, device=DEV)
    rho, amp = R.law(AN, NTAU, DT)
    for frame in (0, 7, (1 << 32) + 7):
        out, z = ops_scenario.noise_force(dev, SEEDS, frame, AN, NTAU, DT, return_draws=True)
        out, z = out.cpu().numpy(), z.cpu().numpy()
        want_out, want_z = R.force(eta, SEEDS, frame, rho, amp)
        assert ulp_close(z, want_z), frame                    # double arithmetic rounded once; the last double bit may differ
        assert np.array_equal(nbits(out), nbits(R.step(eta, rho, amp, z))), frame       # bitwise from the device's own z
        assert np.abs(out - want_out).max() <= 1e-6
        if frame == 7:
            z7 = z
    assert not np.array_equal(z7, z)                           # a frame number >= 2^32 reaches c1
    assert not np.array_equal(z7[0], z7[1]) and not np.array_equal(z7[0], z7[2])       # members read their own seed
    # present == 0 rows are untouched and draw nothing
    out, z = ops_scenario.noise_force(dev, SEEDS, 7, AN, NTAU, DT, present=torch.tensor(present, device=DEV), return_draws=True)
    out, z = out.cpu().numpy(), z.cpu().numpy()
    assert np.array_equal(nbits(out[~present]), nbits(eta[~present])) and (z[~present] == 0).all()
    assert np.array_equal(nbits(z[present]), nbits(z7[present]))
    assert np.array_equal(nbits(out[present]), nbits(R.step(eta, rho, amp, z7)[present]))
    # amp = 0 returns rho eta; noise_tau = 0 returns amp z exactly
    out = ops_scenario.noise_force(dev, SEEDS, 7, 0.0, NTAU, DT).cpu().numpy()
    assert np.array_equal(nbits(out), nbits((rho * eta).astype(np.float32)))
    out = ops_scenario.noise_force(dev, SEEDS, 7, AN, 0.0, DT).cpu().numpy()
    assert np.array_equal(nbits(out), nbits((np.float32(AN) * z7).astype(np.float32)))
    # one member, (N, 2), and in place through the library
    one = ops_scenario.noise_force(dev[1], SEEDS[1], 7, AN, NTAU, DT).cpu().numpy()
    assert np.array_equal(nbits(one), nbits(R.step(eta[1], rho, amp, z7[1])))
    buf = dev.clone()
    sd = torch.tensor([4, 11, -(1 << 63) + 4], device=DEV, dtype=torch.long)
    _lib.check(_lib.lib().piml_noise_force(buf.data_ptr(), None, buf.data_ptr(), None, sd.data_ptr(), len(SEEDS), N, 7,
                                           float(rho), float(amp), torch.cuda.current_stream().cuda_stream), 'piml_noise_force')
    assert np.array_equal(nbits(buf.cpu().numpy()), nbits(R.step(eta, rho, amp, z7)))


# ---- 2. the frame adds the operators' values ----

def run_state(law, walls, groups, noise, grouped, frames=T, use_graph=False, per=4):
    from piml_amd import scenarios
    from piml_amd.models.mlapm import MLAPM as M
    st = scenarios.scenario_state_for(scene(grouped=grouped), frames, CAP, DEV, seeds=SEEDS)
    M._run_scenario(st, law, use_graph, per, walls=walls, groups=groups, noise=noise)
    return scenarios.scenario_result(st)


@functools.lru_cache(maxsize=None)
def forms():
    """the four forms with the term (by-value noise law; left unchanged): name -> (result, walls?, group term?)"""
    from piml_amd import ops_scenario
    S = len(SEEDS)
    law, wall, glaw = ops_scenario.mlapm_law(**PLAIN), ops_scenario.wall_law(AW, BW), ops_scenario.group_law(AG, GDIST)
    ltab = ops_scenario.mlapm_law_table([law] * S, DEV)
    grid = ops_scenario.wall_grid(scene().obstacles, CUTOFF, DEV)
    nl = ops_scenario.noise_law(AN, NTAU, DT)
    return {'plain': (run_state(law, None, None, nl, False), None, False),
            'law table': (run_state(ltab, None, None, nl, False), None, False),
            'walls': (run_state(law, (grid, wall), None, nl, False), grid, False),
            'grouped with walls': (run_state(law, (grid, wall), glaw, nl, True), grid, True)}


@pytest.mark.parametrize('form', ['plain', 'law table', 'walls', 'grouped with walls'])
def test_every_frame_adds_the_operators_noise_to_the_operators_force(form):
    """every recorded frame t, every live slot: acceleration[t + 1] is fadd(F, eta_{t+1}) bitwise, F the existing operators'
    force on frame t's records (one MLAPM step, plus the wall and group forces where present, added in the frame's order), eta
    replayed per slot from its birth with noise_force under frame t's mask; velocity and position follow from acceleration"""
    from piml_amd import ops_scenario
    res, grid, grouped = forms()[form]
    dt = float(res.time_unit)
    assert dt == DT
    eta = torch.zeros(len(SEEDS), CAP, 2, device=DEV)
    checked, felt = 0, 0
    for t in range(T - 1):
        live = res.mask_p[:, t] == 1
        eta = ops_scenario.noise_force(eta, SEEDS, t, AN, NTAU, DT, present=live)
        keep = live & (res.mask_p[:, t + 1] == 1)
        F = torch.stack([_step_fwd(res.position[m, t], res.velocity[m, t], res.desired_speed[m], res.destination[m, t], 'GC',
                                   dt)[1] for m in range(len(SEEDS))])
        if grid is not None:
            F = F + ops_scenario.wall_force(res.position[:, t], grid, AW, BW)
        if grouped:
            F = F + ops_scenario.group_force(res.position[:, t], res.group_first, res.group_size, AG, GDIST)
        a = F + eta
        assert torch.equal(bits(res.acceleration[:, t + 1][keep]), bits(a[keep])), t
        v = res.velocity[:, t] + a * dt
        assert torch.equal(bits(res.velocity[:, t + 1][keep]), bits(v[keep])), t
        assert torch.equal(bits(res.position[:, t + 1][keep]), bits((res.position[:, t] + v * dt)[keep])), t
        checked += int(keep.sum())
        felt += int((eta[keep] != 0).all(-1).sum())
    assert checked > 150 and felt == checked
    assert torch.equal(bits(res.state.noise_state), bits(eta))           # the state the last frame left; unborn slots still 0
    n = torch.tensor([min(s, CAP) for s in res.spawned], device=DEV)
    unborn = torch.arange(CAP, device=DEV)[None] >= n[:, None]
    assert unborn.any() and (res.state.noise_state[unborn] == 0).all()


def test_forms_agree_and_tables_are_read_per_member():
    from piml_amd import ops_scenario
    S = len(SEEDS)
    f = forms()
    assert same_run_fields(f['plain'][0], f['law table'][0])
    law = ops_scenario.mlapm_law(**PLAIN)
    ntab = ops_scenario.noise_law_table([(AN, NTAU)] * S, DT, DEV)
    assert same_run_fields(run_state(law, None, None, ntab, False), f['plain'][0])
    # a table whose rows differ: member m is the by-value run of its row; a row of An = 0 is the run without the term
    rows = [(AN, NTAU), (0.0, 0.0), (0.2, 0.0)]
    mixed = run_state(law, None, None, ops_scenario.noise_law_table(rows, DT, DEV), False)
    assert _same(mixed.member(0), f['plain'][0].member(0))
    assert _same(mixed.member(1), MLAPM(**PLAIN).simulate_scenario(scene(grouped=False), T, seed=SEEDS[1], capacity=CAP))
    assert _same(mixed.member(2), MLAPM(**PLAIN, An=0.2).simulate_scenario(scene(grouped=False), T, seed=SEEDS[2], capacity=CAP))
    assert (mixed.state.noise_state[1] == 0).all() and (mixed.state.noise_state[2, :3] != 0).all()
    with pytest.raises(ValueError):
        run_state(law, None, None, ops_scenario.noise_law_table(rows[:2], DT, DEV), False)
    with pytest.raises(TypeError):
        run_state(law, None, None, (AN, NTAU), False)


def same_run_fields(a, b):
    return all(_same(a.member(m), b.member(m)) for m in range(len(SEEDS)))


# ---- 3. members, captured replays ----

def test_member_of_an_ensemble_is_the_single_run():
    for params, grouped in ((NOISY, False), (dict(NOISY, Ag=AG, group_dist=GDIST, Aw=AW, Bw=BW), True)):
        ens = MLAPM(**params).simulate_ensemble(scene(grouped=grouped), T, SEEDS, capacity=CAP)
        for m, s in enumerate(SEEDS):
            one = MLAPM(**params).simulate_scenario(scene(grouped=grouped), T, seed=s, capacity=CAP)
            assert _same(ens.member(m), one), (m, grouped)
            assert torch.equal(bits(ens.state.noise_state[m]), bits(one.state.noise_state)), (m, grouped)
    assert same_run_fields(ens, forms()['grouped with walls'][0])          # and the model runs the by-value form
    assert not _same(ens.member(0), ens.member(2))                         # the key's high word is read


@pytest.mark.parametrize('frames', [T, T + 1])                # 1 eager + 2 replays of 5; and + 1 eager frame after them
def test_captured_run_is_the_eager_run(frames):
    from piml_amd import hip_graphs_safe
    assert hip_graphs_safe()
    for params, grouped in ((NOISY, False), (dict(NOISY, Ag=AG, group_dist=GDIST, Aw=AW, Bw=BW), True)):
        graph = MLAPM(**params).simulate_ensemble(scene(grouped=grouped), frames, SEEDS, capacity=CAP, use_graph=True,
                                                  frames_per_graph=5)
        eager = MLAPM(**params).simulate_ensemble(scene(grouped=grouped), frames, SEEDS, capacity=CAP, use_graph=False)
        assert same_run_fields(graph, eager), grouped
        assert torch.equal(bits(graph.state.noise_state), bits(eager.state.noise_state)), grouped


# ---- 4. sweeps and the reset ----

def test_sweep_members_are_single_runs_and_a_rerun_starts_from_zero():
    from piml_amd.models.mlapm import SweepRun
    seeds = SEEDS[:2]
    first = [dict(NOISY), dict(PLAIN, An=0.2), dict(PLAIN)]                # two terms that differ, and a candidate without one
    second = [dict(PLAIN, An=1.0, noise_tau=1.0, tau=0.6), dict(PLAIN), dict(PLAIN, An=0.0)]
    sc = scene(grouped=False)
    run = SweepRun(sc, T, 3, seeds, capacity=CAP, use_graph=True, frames_per_graph=4)
    got = []
    for params in (first, first, second, first):
        sw = run.run(params)
        got.append(({k: getattr(sw, k).clone() for k in FIELDS}, list(sw.spawned), list(sw.dropped), run.st.noise_state.clone()))
    assert run.graph is not None and run.noise_table.shape == (6, 2)
    for k in FIELDS:                                          # the same sweep twice, and again after another: the state is reset
        assert torch.equal(bits(got[0][0][k]), bits(got[1][0][k])) and torch.equal(bits(got[0][0][k]), bits(got[3][0][k])), k
    assert torch.equal(bits(got[0][3]), bits(got[1][3])) and torch.equal(bits(got[0][3]), bits(got[3][3]))
    assert not torch.equal(bits(got[0][0]['position']), bits(got[2][0]['position']))
    for params, (fields, spawned, dropped, _) in ((first, got[0]), (second, got[2])):
        for c, p in enumerate(params):
            for k, s in enumerate(seeds):                     # member (c, k) is candidate c's single run under seed k; the
                one = MLAPM(**p).simulate_scenario(sc, T, seed=s, capacity=CAP)     # candidate without An runs the old entry
                m = c * len(seeds) + k
                for name in FIELDS:
                    assert torch.equal(bits(fields[name][m]), bits(getattr(one, name))), (c, k, name)
                assert spawned[m] == one.spawned and dropped[m] == one.dropped
    assert (got[0][3][4:] == 0).all() and (got[2][3][2:] == 0).all()       # members without the term never touch the state
    # a sweep whose first run had no term has no table in its captured frames
    bare = SweepRun(sc, T, 1, seeds, capacity=CAP, use_graph=True, frames_per_graph=4)
    bare.run([dict(PLAIN)])
    assert bare.noise_table is None
    with pytest.raises(ValueError, match='fluctuation'):
        bare.run([dict(NOISY)])
    # the grouped scene with every table at once
    term = dict(NOISY, Ag=AG, group_dist=GDIST, Aw=AW, Bw=BW)
    sw = MLAPM(**PLAIN).simulate_sweep(scene(), T, [term], SEEDS, capacity=CAP)
    assert same_run_fields(sw, forms()['grouped with walls'][0])


# ---- 5. no term, same run; same arrivals ----

def test_zero_strength_and_no_term_are_todays_runs():
    for grouped, extra in ((False, {}), (True, dict(Ag=AG, group_dist=GDIST))):
        today = MLAPM(**PLAIN, **extra).simulate_ensemble(scene(grouped=grouped), T, SEEDS, capacity=CAP)
        zero = MLAPM(**PLAIN, **extra, An=0.0).simulate_ensemble(scene(grouped=grouped), T, SEEDS, capacity=CAP)
        zero_tau = MLAPM(**PLAIN, **extra, An=0.0, noise_tau=NTAU).simulate_ensemble(scene(grouped=grouped), T, SEEDS, capacity=CAP)
        assert today.state.noise_state is None
        for other in (zero, zero_tau):
            assert same_run_fields(other, today), grouped
            assert (other.state.noise_state == 0).all()
        noisy = MLAPM(**NOISY, **extra).simulate_ensemble(scene(grouped=grouped), T, SEEDS, capacity=CAP)
        assert not torch.equal(bits(noisy.position), bits(today.position))
        assert torch.equal(noisy.spawn_count, today.spawn_count) and noisy.spawned == today.spawned and noisy.dropped == today.dropped
        if grouped:
            assert same_arrivals(noisy, today)
        for m in range(len(SEEDS)):                            # what the frame wrote when each agent appeared
            n = min(today.spawned[m], CAP)
            born = (today.mask_p[m][:, :n] == 1).to(torch.uint8).argmax(0)
            assert torch.equal(born, (noisy.mask_p[m][:, :n] == 1).to(torch.uint8).argmax(0))
            idx = torch.arange(n, device=DEV)
            for k in ('position', 'velocity', 'destination'):
                assert torch.equal(bits(getattr(noisy, k)[m][born, idx]), bits(getattr(today, k)[m][born, idx])), (k, m)
            assert torch.equal(bits(noisy.waypoints[m]), bits(today.waypoints[m]))
            assert torch.equal(bits(noisy.desired_speed[m]), bits(today.desired_speed[m]))


def test_single_grouped_run_keeps_its_arrivals():
    a = at_spawn(MLAPM(**NOISY).simulate_scenario(scene(), T, seed=SEEDS[0], capacity=CAP))
    b = at_spawn(MLAPM(**PLAIN).simulate_scenario(scene(), T, seed=SEEDS[0], capacity=CAP))
    assert a['n'] == b['n'] and a['spawned'] == b['spawned'] and a['dropped'] == b['dropped']
    for k in ('born', 'position', 'velocity', 'destination', 'waypoints', 'desired_speed', 'counts', 'group_first', 'group_size'):
        assert np.array_equal(nbits(a[k]) if a[k].dtype == np.float32 else a[k], nbits(b[k]) if b[k].dtype == np.float32 else b[k]), k


# ---- 6. a fit that moves ----

def test_a_small_fit_of_An_to_track_statistics_runs():
    """the plumbing, not identifiability: 2 generations x 4 candidates x 2 seeds against the track statistics of a run made
    with An = 0.5; the objective is finite and does not increase, An stays inside its bounds"""
    import math
    from piml_amd.calibrate import OBJECTIVE_KEYS, calibrate_mlapm_to_stats
    from piml_amd.trackstats import track_stats
    sc = scene(grouped=False)
    made = MLAPM(**PLAIN, An=0.5).simulate_ensemble(sc, T, SEEDS[:2], capacity=CAP)
    ref = track_stats(made.position, made.mask_p, dt=DT, n_lags=T - 1)
    res = calibrate_mlapm_to_stats(sc, (None, None, None, None, ref), init=dict(LAW, An=0.2), fit=('An',), frames=T, seeds=SEEDS[:2],
                                   population=4, generations=2, capacity=CAP, min_count=1)
    print(f'\n[noise] fit: objective {res.initial_loss:.4g} -> {res.final_loss:.4g}, An {res.params["An"]:.4g}; terms {res.terms}')
    assert math.isfinite(res.final_loss) and res.final_loss <= res.initial_loss
    assert all(y <= x for x, y in zip(res.history, res.history[1:])) and len(res.history) == 2
    assert res.params['An'] >= 0.0 and res.params['noise_tau'] == 0.0
    assert set(OBJECTIVE_KEYS['tracks']) <= set(res.terms) and res.seconds['tracks'] > 0
