"""CPU: crowd-dynamics statistics (piml_amd.crowdstats) without a GPU -- argument validation, the numpy restatement
(crowdstats_ref.py) on hand cases, compare_crowd_stats' formulas, the command line's parsing and --box auto, and the C
entry's argument checks (rejected before any HIP call)."""
import json
import math

import numpy as np
import pytest

import crowdstats_ref as REF

R = 0.7
AREA = math.pi * R * R


def test_options_are_validated():
    from piml_amd.crowdstats import check_options
    assert check_options() == (None, None, None)
    box, grid, frames = check_options(box=(0, 10, 0, 4.2), cell=0.5, frames=(2, 9), T=10)
    assert box == (0.0, 10.0, 0.0, 4.2) and grid == (20, 9) and frames == (2, 9)
    for bad in (dict(radius=0), dict(radius=-1), dict(radius=float('nan')), dict(rho_bin=0), dict(rho_bins=0),
                dict(rho_bins=257), dict(rho_bins=2.5), dict(box=(0, 0, 0, 1)), dict(box=(0, 1, 2, 1)),
                dict(box=(0, 1, 0)), dict(box=(0, float('inf'), 0, 1)), dict(box=(0, 1, 0, 1), cell=0),
                dict(frames=(3, 3), T=10), dict(frames=(-1, 3), T=10), dict(frames=(0, 11), T=10)):
        with pytest.raises(ValueError):
            check_options(**bad)


def test_shapes_and_promotion():
    from piml_amd import crowdstats
    with pytest.raises(ValueError):
        crowdstats._promote(np.zeros((2, 3, 2)), np.zeros((2, 3, 2)), np.zeros((2, 4)))
    with pytest.raises(ValueError):
        crowdstats._promote(np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        crowdstats._promote(np.zeros((0, 3, 2)), np.zeros((0, 3, 2)), np.zeros((0, 3)))


def test_grid_shape_matches_the_restatement():
    from piml_amd.crowdstats import grid_shape
    for box, cell in (((5, 25, 15, 35), 0.5), ((0, 1, 0, 1), 0.3), ((-1.1, 2.3, 0.1, 0.2), 0.05)):
        assert grid_shape(box, cell) == REF.grid_shape(box, cell)
    assert grid_shape((0, 1, 0, 1), 0.3) == (4, 4)


def test_lone_agent_and_pair():
    P = np.array([[[1.0, 2.0]]], np.float32)
    st = REF.crowd_stats(P, np.array([[[3.0, 4.0]]], np.float32), np.ones((1, 1), np.float32))
    assert st['density'][0, 0, 0] == np.float32(1 / AREA)
    assert st['n'][0, 0] == 1 and st['n_speed'][0, 0] == 1 and st['sum_speed'][0, 0] == 5.0
    b = int(np.floor(np.float32(1 / AREA) / np.float32(0.25)))
    assert st['fd_count'][0, b] == 1 and st['fd_sum2'][0, b] == 25.0
    d = 0.9
    P = np.array([[[0.0, 0.0], [d, 0.0]]], np.float32)
    st = REF.crowd_stats(P, np.zeros_like(P), np.ones((1, 2), np.float32))
    want = (1 + math.exp(-np.float32(d) ** 2 / R ** 2)) / AREA
    np.testing.assert_allclose(st['density'][0, 0], [want, want], rtol=1e-7)
    # a third agent absent (mask 0) or NaN changes nothing; its velocity never counts
    P3 = np.array([[[0.0, 0.0], [d, 0.0], [0.1, 0.1]]], np.float32)
    for M3, P3b in ((np.array([[1, 1, 0]], np.float32), P3), (np.ones((1, 3), np.float32),
                                                              np.where(np.arange(3)[None, :, None] == 2, np.nan, P3))):
        st3 = REF.crowd_stats(P3b.astype(np.float32), np.zeros_like(P3), M3)
        np.testing.assert_array_equal(st3['density'][0, 0, :2], st['density'][0, 0])
        assert np.isnan(st3['density'][0, 0, 2]) and st3['n'][0, 0] == 2


def test_box_edges_and_non_finite_velocity():
    P = np.array([[[1.0, 1.0], [2.0, 1.0], [1.0, 2.0], [0.0, 0.0]]], np.float32)
    V = np.array([[[1.0, 0.0], [np.nan, 0.0], [0.0, np.inf], [0.0, 2.0]]], np.float32)
    st = REF.crowd_stats(P, V, np.ones((1, 4), np.float32), box=(0, 2, 0, 2), cell=1.0)
    # x == x1 and y == y1 are outside; x == x0 is inside; all four still count as sources
    assert st['n'][0, 0] == 2 and st['n_speed'][0, 0] == 2
    assert np.isnan(st['density'][0, 0, 1]) and np.isnan(st['density'][0, 0, 2])
    assert st['map'][0].tolist() == [[1, 0], [0, 1]]
    st = REF.crowd_stats(P, V, np.ones((1, 4), np.float32))
    assert st['n'][0, 0] == 4 and st['n_speed'][0, 0] == 2 and st['fd_count'].sum() == 2


def _stats(fd_count, fd_sum, sum_speed=(1.0,), n_speed=(1,), sum_density=(1.0,), n=(1,), box=None, mp=None):
    from piml_amd.crowdstats import CrowdStats
    fd_count = np.atleast_2d(fd_count)
    arr = dict(n=np.atleast_2d(n), n_speed=np.atleast_2d(n_speed), sum_speed=np.atleast_2d(sum_speed),
               sum_density=np.atleast_2d(sum_density), fd_count=fd_count, fd_sum=np.atleast_2d(fd_sum),
               fd_sum2=np.atleast_2d(fd_sum) ** 2, map=None if mp is None else np.asarray(mp)[None] if np.ndim(mp) == 2 else mp,
               slices=np.full(fd_count.shape[0], np.atleast_2d(n).shape[1]))
    return CrowdStats(arr, dict(radius=0.7, box=box, cell=0.5, rho_bin=0.25, rho_bins=fd_count.shape[1],
                                frames=(0, np.atleast_2d(n).shape[1])))


def test_compare_formulas():
    from piml_amd.crowdstats import compare_crowd_stats
    a = _stats([100, 60, 10, 0], [100.0, 48.0, 5.0, 0.0], sum_speed=(150.0,), n_speed=(100,), sum_density=(20.0,), n=(10,))
    b = _stats([200, 50, 500, 80], [180.0, 45.0, 100.0, 40.0], sum_speed=(10.0,), n_speed=(20,), sum_density=(9.0,), n=(3,))
    c = compare_crowd_stats(a, b, min_count=50)
    # bins 0 and 1 qualify: w = (100, 50), means (1.0, 0.8) vs (0.9, 0.9)
    want = math.sqrt((100 * 0.1 ** 2 + 50 * 0.1 ** 2) / 150)
    assert c['fd_bins'] == 2 and c['fd_distance'] == pytest.approx(want, rel=1e-12)
    assert c['mean_speed_diff'] == pytest.approx(1.5 - 0.5) and c['mean_density_diff'] == pytest.approx(2.0 - 3.0)
    assert c['map_distance'] is None
    assert math.isnan(compare_crowd_stats(a, b, min_count=1000)['fd_distance'])
    box = (0, 1, 0, 1)
    ma = _stats([1], [1.0], box=box, mp=[[1, 3], [0, 0]])
    mb = _stats([1], [1.0], box=box, mp=[[2, 0], [0, 2]])
    assert compare_crowd_stats(ma, mb, 1)['map_distance'] == pytest.approx(0.25 + 0.75 + 0.0 + 0.5)
    assert compare_crowd_stats(ma, ma, 1)['map_distance'] == 0.0 and compare_crowd_stats(ma, ma, 1)['fd_distance'] == 0.0
    mc = _stats([1], [1.0], box=(0, 2, 0, 1), mp=[[1, 3], [0, 0]])
    assert compare_crowd_stats(ma, mc, 1)['map_distance'] is None


def test_pooled_derived_and_json_round_trip(tmp_path):
    from piml_amd.crowdstats import CrowdStats, merge
    st = _stats([[4, 0], [1, 2]], [[4.0, 0.0], [3.0, 4.0]], sum_speed=[[1.0, 2.0], [3.0, 0.0]], n_speed=[[1, 1], [2, 0]],
                sum_density=[[1.0, 2.0], [3.0, 4.0]], n=[[1, 2], [3, 4]], box=(0, 1, 0, 1),
                mp=np.array([[[2, 0], [0, 0]], [[0, 1], [1, 0]]]))
    p = st.pooled()
    assert p.fd_count.tolist() == [[5, 2]] and p.fd_sum.tolist() == [[7.0, 4.0]] and p.slices.tolist() == [4]
    assert p.n.tolist() == [[4, 6]] and p.map.tolist() == [[[2, 1], [1, 0]]]
    np.testing.assert_allclose(st.fd_mean, [[1.0, np.nan], [3.0, 2.0]])
    np.testing.assert_allclose(st.mean_speed, [[1.0, 2.0], [1.5, np.nan]])
    np.testing.assert_allclose(p.map_density, np.array([[[2, 1], [1, 0]]]) / (4 * 0.25))
    np.testing.assert_allclose(st.fd_std[1], [0.0, 2.0])            # fd_sum2 = fd_sum^2 in _stats: sqrt(9 / 1 - 9), sqrt(16 / 2 - 4)
    d = st.to_json(str(tmp_path / 's.json'))
    back = CrowdStats.from_json(str(tmp_path / 's.json'))
    for k in ('n', 'n_speed', 'sum_speed', 'sum_density', 'fd_count', 'fd_sum', 'fd_sum2', 'map', 'slices'):
        assert np.array_equal(getattr(back, k), getattr(st, k)), k
    assert back.options == st.options and json.loads(json.dumps(d)) == d
    m = merge([st, st])
    assert m.n.shape == (1, 4) and m.fd_count.tolist() == [[10, 4]] and m.slices.tolist() == [8]


def test_cli_parsing_and_auto_box():
    from piml_amd import crowdstats
    a = crowdstats.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'r.npy', '--box', 'auto', '--frames', '3:40',
                             '--radius', '0.5', '--out', 'o.json'])
    assert a.data == ['a.npy', 'b.npy'] and a.ref == 'r.npy' and a.box == 'auto' and a.frames == (3, 40)
    assert a.radius == 0.5 and a.cell == 0.5 and a.out == 'o.json'
    assert crowdstats.get_args(['--data', 'a.npy', '--box', '5,25,15,35']).box == (5.0, 25.0, 15.0, 35.0)
    for bad in (['--data', 'a.npy', '--box', '1,2,3'], ['--data', 'a.npy', '--box', '2,1,0,1'],
                ['--data', 'a.npy', '--frames', '5:5'], ['--data', 'a.npy', '--radius', '0'], ['--box', 'auto']):
        with pytest.raises(SystemExit):
            crowdstats.get_args(bad)
    pos = np.array([[[5.2, 15.1], [24.9, 34.75]], [[np.nan, np.nan], [30.0, 40.0]]], np.float32)
    mask = np.array([[1, 1], [0, 0]], np.float32)
    assert crowdstats.auto_box(pos, mask, 0.5) == (5.0, 25.0, 15.0, 35.0)
    box = crowdstats.auto_box(np.array([[[1.0, 1.0], [2.0, 2.0]]]), np.ones((1, 2)), 0.5)
    assert box == (1.0, 2.5, 1.0, 2.5)                     # an agent on a cell edge stays focal
    with pytest.raises(ValueError):
        crowdstats.auto_box(pos, np.zeros((2, 2)), 0.5)


def test_c_entry_rejects_bad_arguments():
    from piml_amd import _lib
    L = _lib.lib()
    fake = 1 << 20          # never dereferenced: every call below is refused before any HIP call

    def call(S=1, T=2, N=3, t0=0, t1=2, R=0.7, box=0, x1=1., y0=0., h=0.5, gx=2, B=4, mp=fake, wsb=1 << 20, nul=fake):
        return L.piml_crowd_stats(nul, fake, fake, None, S, T, N, t0, t1, R, box, 0., x1, y0, 1., h, gx, 2, 0.25, B,
                                  fake, fake, fake, fake, fake, fake, fake, mp, None, fake, wsb, None)
    for bad in (dict(S=0), dict(T=0), dict(N=0), dict(R=0.0), dict(R=float('inf')), dict(B=0), dict(B=257),
                dict(t0=2, t1=2), dict(t1=3), dict(box=1, x1=0.), dict(box=1, y0=1.), dict(box=1, h=-1.),
                dict(box=1, gx=0), dict(box=1, mp=None), dict(wsb=16), dict(nul=None)):
        assert call(**bad) == 1, bad
    assert L.piml_crowd_stats_workspace_bytes(2, 3, 4) == 2 * 3 * 4 * 20
    assert L.piml_crowd_stats_workspace_bytes(2, -3, 4) == -1
