"""CPU: a recorded clip as an open-world scene (`scenarios.clip_scenario`, spawn law 'clip' = PIML_SPAWN_CLIP): the track
table against the agent-by-agent restatement (tests/scenario_clip_ref.py) on the UCY and GC golden clips, the builder's
errors, the `--scene-from` flags of piml_amd.simulate and the law's id."""
import math
import os
import types

import numpy as np
import pytest
import torch

import scenario_clip_ref as R
from conftest import GOLDEN, bits

CLIPS = ('UCY_Dataset_time162-216_timeunit0.08', 'GC_Dataset_toy1')
_raw = {}


def raw_clip(name):
    """the golden clip as a RawData, loaded once and left unchanged"""
    from piml_amd.data.data import RawData
    if name not in _raw:
        _raw[name] = RawData()
        _raw[name].load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return _raw[name]


def toy_raw(T=6, present=((0, 6), (2, 5)), D=1):
    """a tiny RawData: agent i present in frames present[i] = [a, b), walking +x at 1 m/s towards (10, i)"""
    N = len(present)
    pos = torch.full((T, N, 2), float('nan'))
    mask = torch.zeros(T, N)
    for i, (a, b) in enumerate(present):
        pos[a:b, i, 0] = torch.arange(a, b) * 0.08
        pos[a:b, i, 1] = float(i)
        mask[a:b, i] = 1
    vel = torch.zeros(T, N, 2)
    vel[..., 0] = mask
    way = torch.full((D, N, 2), float('nan'))
    way[0, :, 0], way[0, :, 1] = 10.0, torch.arange(N, dtype=torch.float32)
    return types.SimpleNamespace(position=pos, velocity=vel, mask_p=mask, waypoints=way,
                                 dest_idx=torch.zeros(T, N, dtype=torch.long), obstacles=torch.zeros(0, 2), time_unit=0.08)


def test_law_id():
    from piml_amd import _lib
    assert _lib.SPAWN_LAWS['clip'] == 6
    assert sorted(_lib.SPAWN_LAWS.values()) == list(range(7))


@pytest.mark.parametrize('name', CLIPS)
@pytest.mark.parametrize('window', [None, (40, 300)])
def test_table_of_the_golden_clips(name, window):
    from piml_amd.data.data import desired_speed_per_agent
    from piml_amd.scenarios import Scenario, clip_scenario, default_capacity
    raw = raw_clip(name)
    sc = clip_scenario(raw, frames=window)
    T, N, D = raw.position.shape[0], raw.position.shape[1], raw.waypoints.shape[0]
    a, b = window or (0, T)
    tab = sc.entries.numpy()
    E = tab.shape[0]
    assert isinstance(sc, Scenario) and tab.shape == (E, 3 + D, 2) and tab.dtype == np.float32
    assert sc.spawn_law == 'clip' and sc.arrival_rule == 'radius' and sc.name == 'clip' and sc.num_waypoints == D
    assert sc.time_unit == raw.time_unit and torch.equal(sc.obstacles, raw.obstacles) and sc.spawn_offset == 0.0
    pos, vel, msk = raw.position.numpy(), raw.velocity.numpy(), raw.mask_p.numpy() == 1
    # rows [0, n_initial): exactly the agents of the window's first frame, in clip order, with that frame's state
    at_a = np.nonzero(msk[a])[0]
    assert sc.n_initial == len(at_a) >= 1
    assert np.array_equal(bits(tab[:sc.n_initial, 0]), bits(pos[a, at_a]))
    assert np.array_equal(bits(tab[:sc.n_initial, 1]), bits(vel[a, at_a]))
    # arrival rows: the other tracks of the window, in clip order, at their first in-window position
    later = [i for i in range(N) if msk[a:b, i].any() and not msk[a, i]]
    first = [a + int(np.argmax(msk[a:b, i])) for i in later]
    Ka = E - sc.n_initial
    assert Ka == len(later) and (Ka >= 1 or (name, window) == (CLIPS[1], (40, 300)))   # (the toy's window is closed)
    assert np.array_equal(bits(tab[sc.n_initial:, 0]), bits(pos[first, later]))
    assert np.array_equal(bits(tab[sc.n_initial:, 1]), bits(vel[first, later]))
    # the last non-NaN waypoint of every row is the track's final destination
    agents = list(at_a) + later
    way, num = raw.waypoints.numpy(), raw.dest_num.numpy()
    for r, i in enumerate(agents):
        ok = ~np.isnan(tab[r, 3:]).any(-1)
        assert ok.any() and ok[:ok.sum()].all()                       # waypoints first, NaN after
        assert np.array_equal(tab[r, 3 + ok.sum() - 1], way[num[i] - 1, i])
    # desired speed: the data pipeline's value
    v0 = desired_speed_per_agent(raw.velocity, 25).numpy()
    assert np.array_equal(tab[:, 2, 0], v0[agents]) and (tab[:, 2, 1] == 0).all()
    # rate, thresholds, capacity
    cap = 8 if Ka else 0
    assert sc.fixed_spawn_rate == Ka / (b - a - 1) == sc.spawn_rate and sc.spawn_cap == cap and sc.spawn_cap2 == 0
    thr = sc.poisson_thresholds()
    assert len(thr) == cap and thr == sorted(thr) and all(x <= 1 << 24 for x in thr)
    # default_capacity works from spawn_rate: room for the first frame and the arrivals' 1 - 1e-9 quantile
    want_cap = default_capacity(sc, 200)
    assert sc.n_initial + math.ceil(sc.spawn_rate * 199) <= want_cap <= sc.n_initial + cap * 199
    assert Ka == 0 or want_cap > sc.n_initial
    # and the whole table is the agent-by-agent restatement's (its float64 mean against torch's float32 one: 25 terms)
    want, n0, who, _ = R.table(raw, window)
    assert n0 == sc.n_initial and np.array_equal(who, agents)
    assert np.array_equal(bits(np.delete(tab, 2, 1)), bits(np.delete(want, 2, 1)))
    assert np.allclose(tab[:, 2], want[:, 2], rtol=25 * 2.0 ** -24, atol=0)


def test_waypoints_ahead_only():
    from piml_amd.scenarios import clip_scenario
    raw = toy_raw(T=8, present=((0, 8), (3, 8)), D=3)
    raw.waypoints[1, 0], raw.waypoints[2, 0] = torch.tensor([11.0, 0.0]), torch.tensor([12.0, 0.0])
    raw.waypoints[1, 1] = torch.tensor([11.0, 1.0])
    raw.dest_idx[2:, 0], raw.dest_idx[5:, 0] = 1, 2
    tab = clip_scenario(raw, frames=(2, 8)).entries.numpy()
    assert tab.shape == (2, 6, 2)
    assert np.array_equal(tab[0, 3:5], [[11.0, 0.0], [12.0, 0.0]]) and np.isnan(tab[0, 5]).all()   # waypoint 0 is behind it
    assert np.array_equal(tab[1, 3:5], [[10.0, 1.0], [11.0, 1.0]]) and np.isnan(tab[1, 5]).all()
    # a RawData without dest_idx (ScenarioResult.to_raw_data): the waypoint its destination is
    dest = torch.full((8, 2, 2), float('nan'))
    dest[2:5, 0], dest[5:, 0], dest[3:, 1] = raw.waypoints[1, 0], raw.waypoints[2, 0], raw.waypoints[0, 1]
    del raw.dest_idx
    raw.destination = dest
    assert np.array_equal(bits(clip_scenario(raw, frames=(2, 8)).entries.numpy()), bits(tab))


def test_closed_scene_without_arrivals():
    from piml_amd.scenarios import clip_scenario, default_capacity
    sc = clip_scenario(toy_raw(present=((0, 6), (0, 4))))
    assert sc.n_initial == 2 and sc.entries.shape[0] == 2 and sc.spawn_cap == 0 and sc.spawn_rate == 0
    assert sc.poisson_thresholds() == [] and default_capacity(sc, 100) == 2


def test_builder_errors():
    from piml_amd.scenarios import clip_scenario
    raw = toy_raw()
    assert clip_scenario(raw, frames=(2, 4)).n_initial == 2
    for bad in ((3, 4), (4, 4), (5, 2), (0, 7), (-1, 3)):              # shorter than 2 frames, or outside the clip
        with pytest.raises(ValueError):
            clip_scenario(raw, frames=bad)
    with pytest.raises(ValueError, match='no track'):
        clip_scenario(toy_raw(T=8, present=((0, 3), (6, 8))), frames=(3, 6))
    with pytest.raises(ValueError, match='4096'):
        clip_scenario(toy_raw(T=3, present=((0, 3),) * 4097))
    assert clip_scenario(toy_raw(T=3, present=((0, 3),) * 4096)).n_initial == 4096
    with pytest.raises(ValueError, match='waypoints'):
        clip_scenario(toy_raw(D=9))
    assert clip_scenario(toy_raw(D=8)).entries.shape[1] == 11
    # a rate whose Poisson tail beyond spawn_cap exceeds 1e-6: 30 arrivals in 6 frames
    busy = toy_raw(T=7, present=((0, 7),) + ((1, 7),) * 30)
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(busy)
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(raw, spawn_cap=9)                                 # past the device limit
    # P(K > 1 | 0.2) = 1.75e-2 > 1e-6; P(K > 8 | 0.2) ~ 1e-12
    with pytest.raises(ValueError, match='spawn_cap'):
        clip_scenario(raw, spawn_cap=1)
    assert clip_scenario(raw).fixed_spawn_rate == 1 / 5


def test_restated_rows_cover_every_arrival_row():
    """the integer row map on Ka = 3 (not a power of two) and Ka = 1, independent of the device"""
    rows = R.rows_of(0, np.arange(2, 400), 2, 5)
    assert set(rows.tolist()) == {2, 3, 4} and min(np.bincount(rows)[2:]) > 80
    assert (R.rows_of(7, np.arange(1, 50), 1, 2) == 1).all()
    # the map is monotonic in the 24-bit draw and reaches the last row at its top
    top, Ka = (1 << 24) - 1, 3
    assert (top * Ka) >> 24 == Ka - 1 and (0 * Ka) >> 24 == 0


def test_scene_from_flags(tmp_path, capsys):
    from piml_amd import simulate
    clip = os.path.join(GOLDEN, 'data', CLIPS[0] + '.npy')
    own, _ = simulate.get_args(['--scene-from', clip, '--scene-frames', '10:200', '--scene-jitter', '0.25', '--law', 'mlapm'])
    assert own.scene_from == clip and own.scene_frames == (10, 200) and own.scene_jitter == 0.25 and own.scenario == 'gc'
    own, _ = simulate.get_args(['--scene-from', clip])
    assert own.scene_frames is None and own.scene_jitter == 0.0
    sc = simulate._clip_scene(types.SimpleNamespace(scene_from=clip, scene_frames=(10, 200), scene_jitter=0.25))
    assert sc.spawn_law == 'clip' and sc.spawn_offset == 0.25 and sc.entries.shape[1] == 4
    for bad in (['--scene-from', clip, '--scenario', 'crosswalk'], ['--scene-frames', '0:10'], ['--scene-jitter', '0.1'],
                ['--scene-from', clip, '--scene-frames', '12']):
        with pytest.raises(SystemExit):
            simulate.get_args(bad)
    assert 'not with --scenario' in capsys.readouterr().err
    from piml_amd.scenarios import SCENARIOS
    assert 'clip' not in SCENARIOS                                      # the registry holds the parameter-free scenes only

