"""GPU: the open-world scenario frame (piml_scenario_step / piml_scenario_route) against the reference's route
(tests/golden/scenario_gc.npz) and the numpy restatement of its spawn stream and frame rule (tests/scenario_ref.py), and
`BaseSimulator.simulate_scenario` end to end: graph = eager, determinism, retirement, features, the v2.2 round trip and
the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scenario_ref as R
from conftest import REPO, golden
from test_simulator_gpu import sim_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def gc(**kw):
    from piml_amd.scenarios import gc_scenario
    return gc_scenario(**kw).to(DEV)


def ulps(a, b):
    """max ulp distance of two float32 arrays with equal NaN patterns (asserted)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    ia, ib = a[m].view(np.int32).astype(np.int64), b[m].view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max()) if m.any() else 0


def test_route_matches_reference():
    from piml_amd import ops_scenario
    g = golden('scenario_gc')
    t = lambda k: torch.tensor(g[k], device=DEV)
    r, it = ops_scenario.scenario_route(t('route/o'), t('route/d'), t('pillar'))
    torch.cuda.synchronize()
    assert np.abs(r.cpu().numpy() - g['route/r']).max() <= 1e-5
    assert np.array_equal(it.cpu().numpy(), g['route/iters'])


def _snapshot(st):
    return {k: getattr(st, n).cpu().numpy().copy() for k, n in
            (('p', 'p'), ('v', 'v'), ('a', 'a'), ('dest', 'dest'), ('flag', 'flag'), ('mask', 'mask'),
             ('waypoints', 'waypoints'), ('exit_idx', 'exit_idx'), ('v0', 'desired_speed'))}


def _check_spawned(sc_np, seed, snap, ords, frame_rec, st, f):
    """agents of ordinals `ords` as the restatement spawns them"""
    if len(ords) == 0:
        return
    o, d, v0, _ = R.spawn_agents(seed, ords, sc_np['entries'])
    assert np.array_equal(snap['p'][ords], o), 'spawn origin'
    assert np.array_equal(snap['waypoints'][1, ords], d), 'spawn destination'
    r, it = R.route(o, d, sc_np['pillar'])
    assert np.abs(snap['waypoints'][0, ords] - r).max() <= 1e-5
    assert np.array_equal(st.spawn_iters.cpu().numpy()[ords], it)
    assert np.abs(snap['v0'][ords] - v0).max() <= 1e-6
    assert (snap['flag'][ords] == 0).all() and (snap['mask'][ords] == 1).all()
    assert np.array_equal(snap['dest'][ords], snap['waypoints'][0, ords])
    assert (snap['v'][ords] == 0).all() and (snap['a'][ords] == 0).all()
    for q in range(2):
        assert np.array_equal(snap['exit_idx'][q, ords], R.nearest_entry(snap['waypoints'][q, ords], sc_np['entries']))
    r = frame_rec()
    assert (r['mask'][f, ords] == 1).all() and np.array_equal(r['p'][f, ords], o)


def test_step_matches_restatement_for_400_frames():
    from piml_amd import ops_scenario
    sc = gc()
    sc_np = {'entries': sc.entries.cpu().numpy(), 'pillar': sc.route_polyline.cpu().numpy()}
    seed, T, cap = 7, 400, 1024
    st = ops_scenario.scenario_state(sc, cap, T, seed=seed)
    ops_scenario.scenario_step(st, init=True)
    born, counts = R.schedule(seed, T, sc.n_initial, sc.poisson_thresholds())
    assert len(born) <= cap
    snap = _snapshot(st)
    rec = lambda: {'mask': st.mask_res.cpu().numpy(), 'p': st.p_res.cpu().numpy()}
    _check_spawned(sc_np, seed, snap, np.arange(sc.n_initial), rec, st, 0)
    n = sc.n_initial
    for t in range(T - 1):
        if t < 200:
            a_next = torch.zeros(cap, 2, device=DEV)
        else:                        # a desired-force stand-in: toward the destination at the desired speed, tau = 0.5
            d = torch.nan_to_num(st.dest - st.p)
            e = d / d.norm(dim=-1, keepdim=True).clamp(min=1e-6)
            a_next = ((st.desired_speed.unsqueeze(-1) * e - st.v) / 0.5).contiguous()
        a_np = a_next.cpu().numpy()
        ops_scenario.scenario_step(st, a_next)
        st.t.add_(1)
        new = _snapshot(st)
        want = R.step(snap, a_np, sc_np['entries'], sc.time_unit)
        old = np.arange(n)
        assert np.array_equal(new['flag'][old], want['flag'][old]), t
        assert np.array_equal(new['mask'][old], want['mask'][old]), t
        for k in ('p', 'v', 'a', 'dest'):
            assert ulps(new[k][old], want[k][old]) <= 2, (t, k)
        k = int(counts[t + 1])
        assert int(st.spawn_count[t + 1].item()) == k
        _check_spawned(sc_np, seed, new, np.arange(n, n + k), rec, st, t + 1)
        n += k
        assert int(st.spawned[(t + 1) & 1].item()) == n
        snap = new
    r = rec()
    assert np.array_equal((r['mask'] == 1).argmax(0)[:n], born[:n])      # first frame of every ordinal
    assert (r['mask'][:, n:] == 0).all() and int(st.dropped.item()) == 0
    # a retired agent never reappears
    m = r['mask'][:, :n]
    first = m.argmax(0)
    last = T - 1 - m[::-1].argmax(0)
    assert all(m[first[i]:last[i] + 1, i].all() for i in range(n))
    assert (m[-1] == 0).sum() > 0                                        # agents did leave


def test_small_capacity_drops_exactly_the_restatements_ordinals():
    from piml_amd import ops_scenario
    sc = gc()
    seed, T, cap, pad = 3, 200, 24, 32
    st = ops_scenario.scenario_state(sc, pad, T, seed=seed)
    st.desc.capacity = cap                               # buffers have 32 slots: the tail past 24 x ... is a canary
    before = {k: getattr(st, k).clone() for k in ('p', 'v', 'mask', 'flag', 'p_res', 'mask_res', 'waypoints', 'exit_idx')}
    ops_scenario.scenario_step(st, init=True)
    for _ in range(T - 1):
        ops_scenario.scenario_step(st, torch.zeros(pad, 2, device=DEV))
        st.t.add_(1)
    torch.cuda.synchronize()
    born, counts = R.schedule(seed, T, sc.n_initial, sc.poisson_thresholds())
    total = len(born)
    assert total > cap
    assert int(st.spawned[(T - 1) & 1].item()) == total and int(st.dropped.item()) == total - cap
    assert np.array_equal(st.spawn_count.cpu().numpy(), counts)
    per_slot = {'p': 2, 'v': 2, 'mask': 1, 'flag': 1}
    for k, w in per_slot.items():                        # (capacity, w) state: slots 24 .. 31 untouched
        assert torch.equal(getattr(st, k).reshape(-1)[cap * w:].isnan(), before[k].reshape(-1)[cap * w:].isnan())
        assert torch.equal(torch.nan_to_num(getattr(st, k).reshape(-1)[cap * w:]), torch.nan_to_num(before[k].reshape(-1)[cap * w:]))
    for k, w in (('p_res', T * 2), ('mask_res', T), ('waypoints', 2 * 2), ('exit_idx', 2)):
        a, b = getattr(st, k).reshape(-1)[cap * w:], before[k].reshape(-1)[cap * w:]
        assert torch.equal(torch.nan_to_num(a.float(), 12345.), torch.nan_to_num(b.float(), 12345.)), k
    mask = st.mask_res.reshape(-1)[:T * cap].reshape(T, cap).cpu().numpy()
    assert np.array_equal((mask == 1).argmax(0), born[:cap])


@pytest.fixture(scope='module')
def sim():
    from piml_amd.models.simulators import BaseSimulator
    torch.manual_seed(0)
    s = BaseSimulator(sim_args())
    s.model.eval()
    return s


def _same(a, b):
    for k in ('position', 'velocity', 'acceleration', 'destination', 'mask_p', 'waypoints', 'desired_speed', 'spawn_count'):
        x, y = getattr(a, k), getattr(b, k)
        if not torch.equal(torch.nan_to_num(x, 1e30), torch.nan_to_num(y, 1e30)) or not torch.equal(x.isnan(), y.isnan()):
            return False
    return a.spawned == b.spawned and a.dropped == b.dropped


def test_simulate_scenario_graph_eager_and_seeds(sim):
    sc = gc()
    g = sim.simulate_scenario(sc, 120, seed=5, use_graph=True)
    e = sim.simulate_scenario(sc, 120, seed=5, use_graph=False)
    g2 = sim.simulate_scenario(sc, 120, seed=5)
    assert _same(g, e) and _same(g, g2)
    o = sim.simulate_scenario(sc, 120, seed=6)
    assert not torch.equal(o.spawn_count, g.spawn_count)
    born, counts = R.schedule(5, 120, sc.n_initial, sc.poisson_thresholds())
    assert g.spawned == len(born) and np.array_equal(g.spawn_count.cpu().numpy(), counts)
    m = g.mask_p[:, :g.num_agents].cpu().numpy()
    first, last = m.argmax(0), 119 - m[::-1].argmax(0)
    assert all(m[first[i]:last[i] + 1, i].all() for i in range(m.shape[1]))   # a retired agent never reappears
    assert g.dropped == 0 and torch.isfinite(g.position[:, :g.num_agents][torch.tensor(m == 1, device=DEV)]).all()


def test_simulate_scenario_features_are_the_recorded_states(sim):
    from piml_amd import ops
    a = sim.args
    sc = gc()
    for T in (1, 9, 40):
        res = sim.simulate_scenario(sc, T, seed=2, use_graph=False)
        st = res.state
        t = T - 1
        pf, of, df = ops.relative_features(res.position[t], res.velocity[t], res.acceleration[t], res.destination[t], sc.obstacles,
                                           a.topk_ped, a.sight_angle_ped, a.dist_threshold_ped, a.topk_obs, a.sight_angle_obs,
                                           a.dist_threshold_obs)
        for x, y in ((pf, st.pf), (of, st.of), (df, st.selff[:, :2])):
            assert torch.equal(torch.nan_to_num(x, 1e30), torch.nan_to_num(y, 1e30)), T
        assert torch.equal(st.selff[:, -1], st.desired_speed) and int(st.t.item()) == t


def test_simulate_scenario_round_trip(sim, tmp_path):
    from piml_amd.data.data import RawData, TimeIndexedPedData
    res = sim.simulate_scenario(gc(), 150, seed=9)
    n = res.num_agents
    path = res.save_data(str(tmp_path / 'clip.npy'))
    raw = RawData()
    raw.load_trajectory_data(path)
    T = raw.num_steps
    m = res.mask_p[:T, :n].cpu().numpy()
    assert raw.num_pedestrians == n and np.array_equal(raw.mask_p.numpy(), m)
    assert np.array_equal(raw.position.numpy()[m == 1], res.position[:T, :n].cpu().numpy()[m == 1])
    mem = res.to_raw_data()
    assert torch.equal(mem.mask_p, res.mask_p[:, :n].cpu())
    ds = TimeIndexedPedData()
    ds.make_dataset(sim.args, raw)
    ds.set_dataset_info(ds, raw, list(range(len(ds))))          # as piml_amd.data.dataset builds a clip's rows
    pw = ds.to_pointwise_data()
    assert len(pw) > 100 and torch.isfinite(pw.labels).all()


def test_simulate_cli(tmp_path):
    out = str(tmp_path / 'cli.npy')
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.simulate', '--frames', '200', '--out', out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'spawned' in p.stdout and 'dropped 0' in p.stdout
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(out)
    assert raw.num_pedestrians > 20
