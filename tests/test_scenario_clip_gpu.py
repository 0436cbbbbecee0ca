"""GPU: the clip spawn law of the open-world frame (PIML_SPAWN_CLIP) on a hand-made track table -- E = 5 rows, 2 of them
the first frame's, Ka = 3 arrival rows (not a power of two: the integer row map), D = 2 with one NaN second waypoint --
through every frame entry: spawns bitwise the numpy restatement's (tests/scenario_clip_ref.py), the properties that do not
need it, the ensemble and MLAPM frames, the entry checks and the clip round trip.

Seeds: the spawn parity needs dropped == 0 at capacity 16 over 12 frames at 1.5 arrivals per frame.  The restatement gives
2 + 14 = 16 agents for seed 0, 16 for seed 2 and 14 for seed 2^63 + 3 (17 for seed 1 and 26 for seed 2^63 + 5, which
therefore are not used; one seed keeps the key's top bit set)."""
import ctypes

import numpy as np
import pytest
import torch

import scenario_clip_ref as R
from conftest import bits as nbits
from test_scenario_mlapm_gpu import _same, _step_fwd, bits, mlapm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = [0, 2, (1 << 63) + 3]
NAN = float('nan')
N0, CAP, T = 2, 16, 12
# (position, velocity, (desired speed, 0), waypoint 0, waypoint 1); rows 0..1 walk towards each other 1.5 m apart
TABLE = np.array([
    [[0.0, 0.0], [1.2, 0.0], [1.3, 0.0], [20.0, 0.0], [25.0, 0.0]],
    [[1.5, 0.2], [-1.1, 0.0], [1.25, 0.0], [-20.0, 0.2], [-25.0, 0.2]],
    [[-5.0, 3.0], [1.0, 0.1], [1.1, 0.0], [30.0, 3.0], [35.0, 3.0]],
    [[8.0, -4.0], [0.0, 1.3], [1.4, 0.0], [8.0, 30.0], [NAN, NAN]],
    [[12.0, 6.0], [-0.9, -0.3], [0.95, 0.0], [-30.0, 2.0], [-35.0, 2.0]]], np.float32)


def scene(table=TABLE, n_initial=N0, rate=1.5, spawn_cap=4, jitter=0.0, initial_velocity=True):
    from piml_amd.scenarios import Scenario
    return Scenario(entries=torch.tensor(table), route_polyline=torch.zeros(0, 2), obstacles=torch.zeros(0, 2),
                    time_unit=0.08, n_initial=n_initial, spawn_offset=jitter, arrival_radius=1.0,
                    num_waypoints=table.shape[1] - 3, spawn_cap=spawn_cap, spawn_law='clip', arrival_rule='radius',
                    initial_velocity=initial_velocity, speed_clamp=False, fixed_spawn_rate=rate, name='clip').to(DEV)


def run(sc, cap=CAP, frames=T, **kw):
    """a finished state: the init launch and frames - 1 frames of zero acceleration (seed= or seeds=)"""
    from piml_amd import ops_scenario
    st = ops_scenario.scenario_state(sc, cap, frames, **kw)
    ops_scenario.scenario_step(st, init=True)
    zero = torch.zeros_like(st.a)
    for _ in range(frames - 1):
        ops_scenario.scenario_step(st, zero)
        st.t.add_(1)
    torch.cuda.synchronize()
    return st


def at_spawn(st):
    """what the frame wrote when each slot's agent appeared (numpy): n, born, position, velocity, destination (n, 2),
    waypoints (D, n, 2), desired_speed, counts, spawned, dropped"""
    last = int(st.t.item())
    spawned = int(st.spawned[last & 1].item())
    n = min(spawned, st.capacity)
    m = st.mask_res[:, :n] == 1
    assert bool(m.any(0).all())
    born = m.to(torch.uint8).argmax(0)
    idx = torch.arange(n, device=born.device)
    cpu = lambda x: x.cpu().numpy()
    return dict(n=n, born=cpu(born), position=cpu(st.p_res[born, idx]), velocity=cpu(st.v_res[born, idx]),
                destination=cpu(st.dest_res[born, idx]), acceleration=cpu(st.a_res[born, idx]),
                waypoints=cpu(st.waypoints[:, :n]), desired_speed=cpu(st.desired_speed[:n]),
                counts=cpu(st.spawn_count), spawned=spawned, dropped=int(st.dropped.item()))


def assert_is_replay(got, want):
    assert got['spawned'] == want['spawned'] and got['dropped'] == want['dropped']
    assert np.array_equal(got['counts'], want['counts']) and np.array_equal(got['born'], want['born'])
    for k in ('position', 'velocity', 'waypoints', 'desired_speed'):
        assert np.array_equal(nbits(got[k]), nbits(want[k])), k
    assert np.array_equal(nbits(got['destination']), nbits(want['waypoints'][0]))
    assert (got['acceleration'] == 0).all()


@pytest.fixture(scope='module')
def runs():
    """the 12-frame single run of every seed at capacity 16 (shared, left unchanged)"""
    sc = scene()
    return sc, {s: run(sc, seed=s) for s in SEEDS}


@pytest.mark.parametrize('seed', SEEDS)
def test_spawns_are_the_restatements_bitwise(runs, seed):
    sc, sts = runs
    got = at_spawn(sts[seed])
    want = R.replay(TABLE, N0, seed, T, sc.poisson_thresholds(), CAP)
    assert want['dropped'] == 0 and got['dropped'] == 0 and got['n'] == want['spawned'] > N0 + 3
    assert_is_replay(got, want)
    st = sts[seed]                                             # slots nobody spawned into are untouched
    assert (st.spawn_iters == 0).all()
    assert torch.isnan(st.p[got['n']:]).all() and (st.mask[got['n']:] == 0).all()


def test_initial_velocity_off_and_self_features():
    from piml_amd import ops_scenario
    sc = scene(initial_velocity=False)
    got = at_spawn(run(sc, seed=0))
    want = R.replay(TABLE, N0, 0, T, sc.poisson_thresholds(), CAP, initial_velocity=False)
    assert (want['velocity'] == 0).all()
    assert_is_replay(got, want)
    # the init launch's history / self_features rows: (dest features untouched, history, a = 0, desired speed)
    st = ops_scenario.scenario_state(scene(), CAP, T, hist_width=4, seed=0)
    ops_scenario.scenario_step(st, init=True)
    hist, selff = st.hist[:N0].cpu().numpy(), st.selff[:N0].cpu().numpy()
    assert np.array_equal(hist[:, 2:], TABLE[:N0, 1]) and (hist[:, :2] == 0).all()
    assert np.array_equal(selff[:, 2:6], hist) and (selff[:, 6:8] == 0).all() and np.array_equal(selff[:, 8], TABLE[:N0, 2, 0])
    assert (st.hist[N0:] == 0).all() and (st.selff[N0:] == 0).all()


@pytest.mark.parametrize('seed', SEEDS)
def test_init_places_the_first_rows(runs, seed):
    st = runs[1][seed]
    assert int(st.spawn_count[0]) == N0
    assert np.array_equal(st.p_res[0, :N0].cpu().numpy(), TABLE[:N0, 0])
    assert np.array_equal(st.v_res[0, :N0].cpu().numpy(), TABLE[:N0, 1])
    assert np.array_equal(st.dest_res[0, :N0].cpu().numpy(), TABLE[:N0, 3])
    assert np.array_equal(st.waypoints[:, :N0].cpu().numpy(), TABLE[:N0, 3:].transpose(1, 0, 2))
    assert np.array_equal(st.desired_speed[:N0].cpu().numpy(), TABLE[:N0, 2, 0])
    assert (st.mask_res[0, :N0] == 1).all() and (st.mask_res[0, N0:] == 0).all() and torch.isnan(st.p_res[0, N0:]).all()


def _row_of(got, j, table=TABLE, n_initial=N0):
    """the arrival row that agent j of at_spawn's dict is, exactly (origin, velocity, waypoints, desired speed); -1: none"""
    for r in range(n_initial, table.shape[0]):
        same = np.array_equal(got['position'][j], table[r, 0]) and np.array_equal(got['velocity'][j], table[r, 1]) and \
            got['desired_speed'][j] == table[r, 2, 0] and np.array_equal(nbits(got['waypoints'][:, j]), nbits(table[r, 3:]))
        if same:
            return r
    return -1


def test_every_arrival_is_an_arrival_row_and_every_row_is_drawn(runs):
    for seed in SEEDS:
        got = at_spawn(runs[1][seed])
        assert all(_row_of(got, j) >= N0 for j in range(N0, got['n'])), seed
    got = at_spawn(run(runs[0], cap=512, frames=200, seed=SEEDS[1]))
    assert got['dropped'] == 0 and got['n'] > 200
    rows = [_row_of(got, j) for j in range(N0, got['n'])]
    assert set(rows) == {2, 3, 4}


@pytest.mark.parametrize('seed', SEEDS)
def test_the_count_stream_is_basic_unit1s(runs, seed):
    from piml_amd.scenarios import basic_unit1_scenario
    unit = basic_unit1_scenario()
    unit.fixed_spawn_rate, unit.spawn_cap = 1.5, 4
    sc = runs[0]
    assert unit.poisson_thresholds() == sc.poisson_thresholds()
    want = run(unit.to(DEV), cap=64, seed=seed).spawn_count
    assert torch.equal(runs[1][seed].spawn_count[1:], want[1:]) and int(want[0]) == 1


@pytest.mark.parametrize('seed', SEEDS)
def test_jitter(seed):
    sc = scene(jitter=0.25)
    got = at_spawn(run(sc, seed=seed))
    want = R.replay(TABLE, N0, seed, T, sc.poisson_thresholds(), CAP, jitter=0.25)
    assert_is_replay(got, want)
    assert np.array_equal(got['position'][:N0], TABLE[:N0, 0])                 # frame 0 is not jittered
    off = got['position'][N0:] - TABLE[want['row'][N0:], 0]
    # |0.25 (2u - 1)| <= 0.25 exactly; the sum rounds once, half an ulp of a coordinate below 16: 2^-21
    assert np.abs(off).max() <= 0.25 + 2.0 ** -21 and (off != 0).any(1).all()


def test_a_single_arrival_row():
    table = TABLE[[0, 1, 3]]
    got = at_spawn(run(scene(table), seed=SEEDS[2]))
    assert got['n'] > N0 + 3
    assert all(_row_of(got, j, table) == 2 for j in range(N0, got['n']))


def test_capacity_drops_and_never_writes_past_it():
    """a descriptor of capacity 3 over buffers of 16 slots: whatever lies past the 3-slot layout keeps its initial value"""
    from piml_amd import _lib, ops, ops_scenario
    sc = scene()
    st = ops_scenario.scenario_state(sc, CAP, T, seed=0)
    desc = _lib.Scenario.from_buffer_copy(st.desc)
    desc.capacity = 3
    zero = torch.zeros(CAP, 2, device=DEV)
    with torch.cuda.device(DEV):
        for t in range(T):
            _lib.check(_lib.lib().piml_scenario_step_members(ctypes.byref(desc), ctypes.byref(st.rules), 1, ops._ptr(st.seeds),
                                                             ops._ptr(zero) if t else None, int(t == 0), ops._stream()), 'frame')
            if t:
                st.t.add_(1)
    torch.cuda.synchronize()
    want = R.replay(TABLE, N0, 0, T, sc.poisson_thresholds(), 3)
    assert want['spawned'] == 16 and int(st.spawned[(T - 1) & 1]) == 16 and int(st.dropped) == 13 == want['dropped']
    assert np.array_equal(st.spawn_count.cpu().numpy(), want['counts'])
    D, hw = 2, 2
    assert np.array_equal(nbits(st.waypoints.view(-1)[:D * 3 * 2].view(D, 3, 2).cpu().numpy()), nbits(want['waypoints']))
    for name, used, nan in (('p', 3 * 2, True), ('dest', 3 * 2, True), ('v', 3 * 2, False), ('a', 3 * 2, False),
                            ('mask', 3, False), ('desired_speed', 3, False), ('flag', 3, False), ('hist', 3 * hw, False),
                            ('selff', 3 * (hw + 5), False), ('waypoints', D * 3 * 2, True), ('spawn_iters', 3, False),
                            ('p_res', T * 3 * 2, True), ('dest_res', T * 3 * 2, True), ('v_res', T * 3 * 2, False),
                            ('a_res', T * 3 * 2, False), ('mask_res', T * 3, False)):
        rest = getattr(st, name).view(-1)[used:]
        assert bool(torch.isnan(rest).all() if nan else (rest == 0).all()), name


def test_members_and_the_rules_entry_are_bitwise_the_single_run(runs):
    from piml_amd import _lib, ops, ops_scenario
    sc, sts = runs
    ens = run(sc, seeds=SEEDS)
    names = ('p', 'v', 'a', 'dest', 'hist', 'selff', 'desired_speed', 'mask', 'flag', 'waypoints', 'spawn_iters', 'p_res',
             'v_res', 'a_res', 'dest_res', 'mask_res', 'spawn_count', 'spawned')
    for m, s in enumerate(SEEDS):
        for k in names:
            assert torch.equal(bits(getattr(ens, k)[m]), bits(getattr(sts[s], k))), (s, k)
        assert int(ens.dropped[m]) == int(sts[s].dropped) == 0
    # piml_scenario_step_rules takes the law too (key = the descriptor's seed)
    st = ops_scenario.scenario_state(sc, CAP, T, seed=SEEDS[2])
    zero = torch.zeros(CAP, 2, device=DEV)
    with torch.cuda.device(DEV):
        for t in range(T):
            _lib.check(_lib.lib().piml_scenario_step_rules(ctypes.byref(st.desc), ctypes.byref(st.rules),
                                                           ops._ptr(zero) if t else None, int(t == 0), ops._stream()), 'rules')
            if t:
                st.t.add_(1)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(bits(getattr(st, k)), bits(getattr(sts[SEEDS[2]], k))), k


def test_mlapm_frame():
    sc = scene()
    law = mlapm('GC')
    ens = law.simulate_ensemble(sc, T, SEEDS)
    one = [law.simulate_scenario(sc, T, seed=s, capacity=ens.capacity) for s in SEEDS]
    for m, s in enumerate(SEEDS):
        assert _same(ens.member(m), one[m]), s
        want = R.replay(TABLE, N0, s, T, sc.poisson_thresholds(), ens.capacity)      # the network path's arrivals
        assert one[m].spawned == want['spawned'] and one[m].dropped == 0
        assert np.array_equal(one[m].spawn_count.cpu().numpy(), want['counts'])
        assert np.array_equal(nbits(one[m].waypoints[:, :one[m].num_agents].cpu().numpy()), nbits(want['waypoints']))
    # frame 1 is MLAPM.step on frame 0's agents (piml_mlapm_step_fwd over all capacity rows, absent ones NaN and skipped)
    res, dt = one[0], float(sc.time_unit)
    keep = (res.mask_p[0] == 1) & (res.mask_p[1] == 1)
    assert keep.tolist() == [True] * N0 + [False] * (ens.capacity - N0)
    act, frc = _step_fwd(res.position[0], res.velocity[0], res.desired_speed, res.destination[0], 'GC', dt)
    assert torch.equal(bits(res.velocity[1][keep]), bits(act[keep]))
    assert torch.equal(bits(res.position[1][keep]), bits(res.position[0][keep] + act[keep] * dt))
    assert torch.equal(bits(res.acceleration[1][keep]), bits(frc[keep]))
    free = (torch.tensor(TABLE[:N0, 2, :1], device=DEV) * torch.nn.functional.normalize(
        res.destination[0][keep] - res.position[0][keep], dim=-1) - res.velocity[0][keep]) / 0.5
    assert (frc[keep] - free).norm(dim=-1).min() > 1e-3            # the two agents do feel each other


def test_entry_checks():
    from piml_amd import _lib, ops_scenario
    sc = scene()
    st = ops_scenario.scenario_state(sc, CAP, T, seed=1)
    L = _lib.lib()
    watched = ('p', 'v', 'mask', 'waypoints', 'p_res', 'mask_res', 'spawn_count', 'spawned', 'dropped')
    before = [getattr(st, k).clone() for k in watched]
    zero = torch.zeros(CAP, 2, device=DEV)
    law = ops_scenario.mlapm_law()

    def codes(desc=st.desc, rules=st.rules):
        d, r, sd = ctypes.byref(desc), ctypes.byref(rules), st.seeds.data_ptr()
        return (L.piml_scenario_step_rules(d, r, None, 1, None), L.piml_scenario_step_members(d, r, 1, sd, None, 1, None),
                L.piml_scenario_step_members(d, r, 1, sd, zero.data_ptr(), 0, None),
                L.piml_scenario_step_mlapm(d, r, 1, sd, ctypes.byref(law), 0, None))

    def broken(**kw):
        d = _lib.Scenario.from_buffer_copy(st.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    two = _lib.ScenarioRules.from_buffer_copy(st.rules)
    two.spawn_cap2 = 1
    gc_rule = _lib.ScenarioRules.from_buffer_copy(st.rules)
    gc_rule.arrival_rule = _lib.ARRIVAL_RULES['gc']
    cases = {'P != 3 + D': dict(desc=broken(P=4)), 'P != 3 + D (D)': dict(desc=broken(D=1)),
             'NULL entries': dict(desc=broken(entries=None)), 'n_initial > E': dict(desc=broken(n_initial=6)),
             'Ka == 0 with spawn_cap > 0': dict(desc=broken(n_initial=5)), 'spawn_cap2 != 0': dict(rules=two),
             'more than 2^24 arrival rows': dict(desc=broken(E=(1 << 24) + N0 + 1)), 'GC arrival rule': dict(rules=gc_rule)}
    for what, kw in cases.items():
        assert codes(**kw) == (1, 1, 1, 1), what
        with pytest.raises(_lib.PimlHipError):
            _lib.check(codes(**kw)[0], what)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(getattr(st, k))) for x, k in zip(before, watched))   # nothing was launched
    # Ka == 0 is a closed scene once spawn_cap is 0, and the untouched descriptor is accepted
    closed = broken(n_initial=5, spawn_cap=0)
    assert L.piml_scenario_step_members(ctypes.byref(closed), ctypes.byref(st.rules), 1, st.seeds.data_ptr(), None, 1, None) == 0
    torch.cuda.synchronize()
    assert int(st.spawned[0]) == 5 and np.array_equal(st.p[:5].cpu().numpy(), TABLE[:, 0])


def test_a_simulated_clip_is_again_a_scene(tmp_path):
    """save_data -> load_trajectory_data -> clip_scenario.  The builder refuses a rate whose Poisson tail beyond spawn_cap
    = 8 exceeds 1e-6, and a 12-frame clip recorded at 1.5 arrivals per frame has one (P(K > 8 | 1.5) = 2.6e-5), so this
    scene arrives at 0.5 per frame (P(K > 8 | 1) = 1.1e-6 is the edge: at most 10 arrivals in the 11 frames)."""
    from piml_amd.data.data import RawData
    from piml_amd.scenarios import clip_scenario
    sc = scene(rate=0.5)
    res = mlapm('GC').simulate_scenario(sc, T, seed=SEEDS[1])
    n = res.num_agents
    assert N0 < n <= N0 + 10 and res.dropped == 0
    raw = RawData()
    raw.load_trajectory_data(res.save_data(str(tmp_path / 'clip.npy')))
    assert raw.num_pedestrians == n
    again = clip_scenario(raw)
    tab = again.entries.numpy()
    # (a v2.2 clip keeps the waypoints its agents reached or were heading for: nobody gets past waypoint 0 in 12 frames)
    assert raw.num_destinations == 1 and again.num_waypoints == 1
    assert again.n_initial == N0 and tab.shape == (n, 4, 2) and again.spawn_law == 'clip'
    assert np.array_equal(tab[:N0, 3], TABLE[:N0, 3])
    assert np.array_equal(tab[:N0, 0], TABLE[:N0, 0])
    first = (res.mask_p[:, :n] == 1).to(torch.uint8).argmax(0)
    assert np.array_equal(tab[:, 0], res.position[first, torch.arange(n, device=first.device)].cpu().numpy())
    assert again.fixed_spawn_rate == (n - N0) / (raw.num_steps - 1)
    again = again.to(DEV)
    assert at_spawn(run(again, cap=32, frames=6, seed=0))['n'] >= N0           # and it runs
