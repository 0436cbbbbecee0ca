"""CPU: the open-world scenario's data side against the reference's GC scenario, route and clip writer
(tests/golden/scenario_gc.npz, tests/golden/make_scenario_gc.py), the numpy restatement of the device's spawn stream
(tests/scenario_ref.py), and the C ABI's argument checks of piml_scenario_step / piml_scenario_route (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scenario_ref as R
from conftest import golden
from philox_ref import philox4x32_10


def test_gc_geometry_is_the_references_bit_for_bit():
    from piml_amd.scenarios import gc_scenario
    g = golden('scenario_gc')
    sc = gc_scenario()
    assert g['wall'].shape == (3994, 2) and g['pillar'].shape == (100, 2) and g['entries'].shape == (7, 100, 2)
    assert np.array_equal(sc.obstacles.numpy(), np.concatenate((g['wall'], g['pillar'])))
    assert np.array_equal(sc.route_polyline.numpy(), g['pillar'])
    assert np.array_equal(sc.entries.numpy(), g['entries'])
    assert sc.n_initial == 20 and sc.num_waypoints == 2 and sc.spawn_rate == 5 * 0.08
    assert gc_scenario(time_unit=0.1, uniform_desired_speed=True).uniform_desired_speed


def test_spawn_stream_philox_is_the_known_answer():
    # Random123 known-answer vector of philox4x32-10 (zero counter, zero key), which philox_ref.py restates
    assert [int(x) for x in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    w = R._words(0, np.array([0, 7]), 1)
    ref = philox4x32_10(np.array([0, 7], np.uint64), 0, 0, R.STREAM | 1, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(w, ref))


def test_spawn_counts_are_poisson_04():
    from piml_amd.scenarios import gc_scenario
    sc = gc_scenario()
    thr = sc.poisson_thresholds()
    assert len(thr) == 8 and thr == sorted(thr) and thr[-1] <= 1 << 24
    n = 100000
    k = R.spawn_counts(3, np.arange(1, n + 1), thr)
    lam = 0.4
    # mean and variance within 4 sigma (var of the sample variance of Poisson: (lam + 2 lam^2 (n/(n-1))) / n ~ (lam + 2 lam^2) / n)
    assert abs(k.mean() - lam) < 4 * np.sqrt(lam / n)
    assert abs(k.var() - lam) < 4 * np.sqrt((lam + 2 * lam * lam) / n)
    assert k.max() <= 8
    assert not np.array_equal(k[:1000], R.spawn_counts(4, np.arange(1, 1001), thr))       # the seed matters


def test_spawn_draws_are_distinct_and_in_range():
    from piml_amd.scenarios import gc_scenario
    ent = gc_scenario().entries.numpy()
    dr = R.agent_draws(11, np.arange(20000), 7, 100)
    assert (dr['oe'] != dr['de']).all()
    for k, m in (('oe', 7), ('de', 7), ('oi', 100), ('di', 100)):
        assert dr[k].min() == 0 and dr[k].max() == m - 1
    pairs = np.bincount(dr['oe'] * 7 + dr['de'], minlength=49).reshape(7, 7)
    assert (np.diag(pairs) == 0).all() and pairs[~np.eye(7, dtype=bool)].min() > 0.8 * 20000 / 42
    assert 0 <= dr['uo'].min() and dr['uo'].max() < 1 and abs(dr['z'].mean()) < 0.05 and abs(dr['z'].std() - 1) < 0.05
    o, d, v0, _ = R.spawn_agents(11, np.arange(1000), ent)
    assert v0.min() >= np.float32(0.7) and abs(float(np.median(v0)) - 1.34) < 0.05
    _, _, v1, _ = R.spawn_agents(11, np.arange(10), ent, uniform=True)
    assert (v1 == np.float32(1.34)).all()


def test_route_restatement_matches_the_reference():
    g = golden('scenario_gc')
    r, it = R.route(g['route/o'], g['route/d'], g['pillar'])
    assert np.abs(r - g['route/r']).max() <= 1e-5
    assert np.array_equal(it, g['route/iters']) and it.max() < 16
    assert (it > 0).sum() > 100                        # pairs that do cross the pillar


def test_default_capacity():
    from piml_amd.scenarios import gc_scenario, default_capacity
    sc = gc_scenario()
    c = default_capacity(sc, 750)
    mu = 0.4 * 749
    assert 20 + mu + 4 * np.sqrt(mu) < c < 20 + mu + 9 * np.sqrt(mu)
    assert default_capacity(sc, 1) == 20 and default_capacity(sc, 2) <= 20 + 8


def _clip_rows(traj, dest):
    t = np.array([(a, x, y, f) for a, tr in enumerate(traj) for (x, y, f) in tr], np.float64)
    d = np.array([(a, x, y, f) for a, ds in enumerate(dest) for (x, y, f) in ds], np.float64)
    return t, d


def test_save_clip_reproduces_the_references_tuple(tmp_path):
    from piml_amd.data.data import RawData
    from piml_amd.scenarios import clip_tuple, save_clip
    g = golden('scenario_gc')
    args = (g['clip/position'], g['clip/mask_p'], g['clip/waypoints'], g['clip/destination'], g['clip/obstacles'])
    meta, traj, dest, obs = clip_tuple(*args, {'time_unit': 0.08})
    assert meta == {'time_unit': 0.08, 'version': 'v2.2'}
    assert [len(t) for t in traj] == g['clip/traj_len'].tolist()
    assert [len(d) for d in dest] == g['clip/dest_len'].tolist()
    t, d = _clip_rows(traj, dest)
    assert np.array_equal(t, g['clip/traj']) and np.array_equal(d, g['clip/dest'])
    assert all(type(x) is float and type(y) is float and type(f) is int for tr in traj for (x, y, f) in tr)
    assert all(type(f) is int for ds in dest for (_, _, f) in ds)
    assert np.array_equal(np.array(obs), g['clip/obstacles_list'])
    path = save_clip(str(tmp_path / 'clip.npy'), *args, {'time_unit': 0.08})
    raw = RawData()
    raw.load_trajectory_data(path)
    m = g['clip/mask_p'] == 1
    assert np.array_equal(raw.mask_p.numpy() == 1, m)
    assert np.array_equal(raw.position.numpy()[m], g['clip/position'][m])
    assert raw.num_destinations == 2 and raw.time_unit == 0.08


def test_scenario_abi_checks_without_gpu():
    from piml_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 35 and L.piml_abi_version() == 35
    assert L.piml_scenario_step(None, None, 0, None) == 1
    s = _lib.Scenario()                                 # all-zero descriptor: capacity 0
    assert L.piml_scenario_step(ctypes.byref(s), None, 1, None) == 1
    assert L.piml_scenario_route(None, None, 0, None, 100, 16, 2.0, None, None, None) == 0       # empty: no-op
    assert L.piml_scenario_route(None, None, 4, None, 1, 16, 2.0, None, None, None) == 1         # R < 2
    assert L.piml_scenario_route(None, None, 4, None, 100, 65, 2.0, None, None, None) == 1       # iteration cap
    assert L.piml_scenario_route(None, None, 4, None, 100, 16, 2.0, None, None, None) == 1       # NULL buffers


def test_scenario_ops_refuse_cpu_tensors():
    from piml_amd import _lib, ops_scenario
    from piml_amd.scenarios import gc_scenario
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.scenario_route(torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(5, 2))
    with pytest.raises(_lib.PimlHipError):
        ops_scenario.scenario_state(gc_scenario(), 64, 10)
