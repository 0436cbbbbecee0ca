"""CPU: the Voronoi density of the crowd statistics.  The numpy restatement of the cell (voronoi_ref.py)
against scipy's Voronoi diagram and against the partition property; option checking, the JSON round trip (a file written
before the option existed included), compare / merge refusing mixed densities, the command lines' flags and the C ABI's
argument checks."""
import ctypes
import json

import numpy as np
import pytest

import voronoi_ref as VREF


def _points(n, side, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 2)) * side).astype(np.float32)


def test_restatement_against_scipy():
    """Cells that neither the cut-off polygon nor (there are none) bounds touch are the scipy regions: 1e-9 relative, both
    sides float64 -- a check of the definition (clip order, skip rules, intersection formula), not of precision."""
    spatial = pytest.importorskip('scipy.spatial')
    from piml_amd.crowdstats import voronoi_dirs
    P = _points(250, 10.0, seed=3)
    cutoff, sides = 4.0, 16
    area, verts, _ = VREF.cells(P, np.ones(len(P)), cutoff, voronoi_dirs(sides))
    vor = spatial.Voronoi(P.astype(np.float64))
    inner = cutoff * np.cos(np.pi / sides)                         # the polygon's inscribed circle
    checked = 0
    for i, reg in enumerate(vor.point_region):
        idx = vor.regions[reg]
        if not idx or -1 in idx:
            continue
        v = vor.vertices[idx] - P[i].astype(np.float64)
        if np.hypot(v[:, 0], v[:, 1]).max() >= 0.999 * inner:
            continue
        v = v[np.argsort(np.arctan2(v[:, 1], v[:, 0]))]
        want = VREF.shoelace(v)
        assert abs(area[i] - want) <= 1e-9 * want, (i, area[i], want)
        assert verts[i] == len(idx)
        checked += 1
    assert checked > 150


@pytest.mark.parametrize('n', [1, 2, 65, 300])
def test_restatement_partitions_the_bounds(n):
    from piml_amd.crowdstats import voronoi_dirs
    bounds = (2.0, 14.0, -3.0, 6.0)
    P = _points(n, 1.0, seed=n) * np.float32([12.0, 9.0]) + np.float32([2.0, -3.0])
    area, _, _ = VREF.cells(P, np.ones(n), 1e3, voronoi_dirs(), bounds=bounds)
    assert np.isfinite(area).all() and (area > 0).all()
    assert abs(area.sum() - 108.0) <= 1e-9 * 108.0


def test_restatement_skip_rules_and_focal_set():
    from piml_amd.crowdstats import voronoi_dirs
    d = voronoi_dirs(16)
    full = 8.0 * np.sin(2 * np.pi / 16)
    P = np.float32([[0, 0], [0, 0], [2.0, 0], [0.5, 0.5], [np.nan, 0], [9, 9]])
    M = np.float32([1, 1, 1, 0, 1, 1])
    area, verts, peak = VREF.cells(P, M, 1.0, d, bounds=(-5, 5, -5, 5))
    # coincident agents share the whole cell; a neighbour at exactly 2 cutoff, an absent one and a NaN one do not cut;
    # an agent outside the bounds is not focal
    assert area[0] == area[1] == pytest.approx(full, rel=1e-7) and area[2] == pytest.approx(full, rel=1e-7)
    assert np.isnan(area[3:]).all() and verts[0] == 16 and peak[0] == 16
    area, _, _ = VREF.cells(P, M, 1.0, d, n_active=1)
    assert np.isfinite(area).tolist() == [True] + [False] * 5
    a32, _, _ = VREF.cells(P, M, 1.0, d, dtype=np.float32)
    assert a32[0] == pytest.approx(full, rel=1e-6)


def test_options_are_validated():
    from piml_amd.crowdstats import check_density, check_options, voronoi_dirs
    assert check_density() == ('gaussian', None, None, None)
    assert check_density('voronoi') == ('voronoi', 1.0, None, 16)
    assert check_density('voronoi', 0.8, (0, 1, 2, 3.5), 12) == ('voronoi', 0.8, (0.0, 1.0, 2.0, 3.5), 12)
    assert check_options(density='voronoi', cutoff=2.0, bounds=(0, 1, 0, 1)) == (None, None, None)
    for bad in (dict(density='kernel'), dict(cutoff=1.0), dict(bounds=(0, 1, 0, 1)), dict(sides=16),
                dict(density='voronoi', cutoff=0.0), dict(density='voronoi', cutoff=float('nan')),
                dict(density='voronoi', cutoff=float('inf')), dict(density='voronoi', sides=2),
                dict(density='voronoi', sides=33), dict(density='voronoi', sides=7.5), dict(density='voronoi', sides=True),
                dict(density='voronoi', bounds=(0, 1, 0)), dict(density='voronoi', bounds=(1, 1, 0, 1)),
                dict(density='voronoi', bounds=(0, 1, 0, float('inf')))):
        with pytest.raises(ValueError):
            check_density(**bad)
        with pytest.raises(ValueError):
            check_options(**bad)
    d = voronoi_dirs(16)
    ang = 2 * np.pi * np.arange(16) / 16
    assert d.dtype == np.float32 and d.shape == (16, 2)
    assert np.array_equal(d, np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))


def _stats(density=None, dropped=None, **opts):
    from piml_amd.crowdstats import CrowdStats
    arr = dict(n=[[3, 4], [5, 6]], n_speed=[[3, 4], [5, 5]], sum_speed=[[3.0, 4.0], [5.0, 5.5]],
               sum_density=[[1.0, 2.0], [3.0, 4.0]], fd_count=[[60, 70], [80, 90]], fd_sum=[[60.0, 35.0], [80.0, 45.0]],
               fd_sum2=[[60.0, 20.0], [80.0, 30.0]], map=None, slices=[2, 2])
    if dropped is not None:
        arr['dropped'] = dropped
    options = dict(radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=2, frames=(0, 2), **opts)
    if density is not None:
        options['density'] = density
    return CrowdStats(arr, options)


VOR = dict(cutoff=1.0, bounds=(0.0, 4.0, 0.0, 4.0), sides=16)


def test_dropped_and_options_are_carried(tmp_path):
    from piml_amd.crowdstats import CrowdStats, call_options, merge
    g = _stats()
    assert g.options['density'] == 'gaussian' and g.options['cutoff'] is None and g.options['bounds'] is None
    assert g.dropped.tolist() == [0, 0]
    v = _stats('voronoi', dropped=[1, 2], **VOR)
    assert v.pooled().dropped.tolist() == [3] and v.member(1).dropped.tolist() == [2]
    assert v.select([1, 1, 0]).dropped.tolist() == [2, 2, 1] and v.select([1]).options == v.options
    assert merge([v, v]).dropped.tolist() == [6] and merge([v, v]).options['density'] == 'voronoi'
    d = v.to_json(str(tmp_path / 'v.json'))
    assert json.loads(json.dumps(d)) == d and d['options']['density'] == 'voronoi' and d['options']['bounds'] == [0, 4, 0, 4]
    back = CrowdStats.from_json(str(tmp_path / 'v.json'))
    assert back.options == v.options and back.dropped.tolist() == [1, 2]
    assert call_options(v) == dict(radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=2, density='voronoi', **VOR)
    assert call_options(g) == dict(radius=0.7, box=None, cell=0.5, rho_bin=0.25, rho_bins=2)
    # a file written before there was a second density: no density keys, no dropped array
    old = g.to_json()
    for k in ('density', 'cutoff', 'bounds', 'sides'):
        del old['options'][k]
    del old['arrays']['dropped']
    back = CrowdStats.from_json(json.loads(json.dumps(old)))
    assert back.options == g.options and back.options['density'] == 'gaussian' and back.dropped.tolist() == [0, 0]


def test_mixed_densities_are_refused():
    from piml_amd.crowdstats import compare_crowd_stats, merge
    g, v = _stats(), _stats('voronoi', **VOR)
    assert compare_crowd_stats(v, v, 1)['fd_distance'] == 0.0
    others = (g, _stats('voronoi', **{**VOR, 'cutoff': 1.5}), _stats('voronoi', **{**VOR, 'bounds': None}),
              _stats('voronoi', **{**VOR, 'bounds': (0.0, 4.0, 0.0, 5.0)}))
    for other in others:
        with pytest.raises(ValueError):
            compare_crowd_stats(v, other, 1)
        with pytest.raises(ValueError):
            compare_crowd_stats(other, v, 1)
        with pytest.raises(ValueError):
            merge([v, other])
    assert compare_crowd_stats(g, _stats(), 1)['fd_distance'] == 0.0      # two Gaussian sides compare as before


def test_command_line_flags():
    from piml_amd import calibrate, crowdstats, simulate
    a = crowdstats.get_args(['--data', 'a.npy', '--density', 'voronoi', '--cutoff', '0.8', '--box', 'auto', '--bounds', 'auto'])
    assert a.density == 'voronoi' and a.cutoff == 0.8 and a.bounds == 'auto'
    a = crowdstats.get_args(['--data', 'a.npy', '--density', 'voronoi', '--bounds', '5,25,15,35'])
    assert a.bounds == (5.0, 25.0, 15.0, 35.0) and a.cutoff is None
    assert crowdstats.get_args(['--data', 'a.npy']).density == 'gaussian'
    for bad in (['--cutoff', '1.0'], ['--bounds', '0,1,0,1'], ['--density', 'voronoi', '--cutoff', '0'],
                ['--density', 'voronoi', '--bounds', 'auto'], ['--density', 'voronoi', '--bounds', '1,0,0,1'],
                ['--density', 'delaunay']):
        with pytest.raises(SystemExit):
            crowdstats.get_args(['--data', 'a.npy'] + bad)
    own, _ = simulate.get_args(['--law', 'mlapm', '--seeds', '0:2', '--stats', 's.json', '--stats-density', 'voronoi',
                                '--stats-cutoff', '1.5'])
    assert simulate._crowd_kw(own) == dict(density='voronoi', cutoff=1.5)
    own, _ = simulate.get_args(['--law', 'mlapm', '--seeds', '0:2', '--stats', 's.json'])
    assert simulate._crowd_kw(own) == {}
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'mlapm', '--stats', 's.json', '--stats-cutoff', '1.5'])
    a = calibrate.get_args(['--data', 'c.npy', '--match-stats', '--stats-density', 'voronoi', '--stats-cutoff', '0.9'])
    assert a.stats_density == 'voronoi' and a.stats_cutoff == 0.9
    with pytest.raises(SystemExit):
        calibrate.get_args(['--data', 'c.npy', '--match-stats', '--stats-cutoff', '0.9'])


def test_library_checks_arguments_before_any_launch():
    """hipErrorInvalidValue without touching the device: every call below is refused, so the (non-NULL, never
    dereferenced) stand-ins for device pointers are not read."""
    from piml_amd import _lib
    L = _lib.lib()
    assert 'piml_crowd_stats_voronoi' in _lib.SIGNATURES and 'piml_crowd_stats_voronoi_workspace_bytes' in _lib.SIGNATURES
    assert L.piml_crowd_stats_voronoi_workspace_bytes(2, 3, 5, 4) == 2 * 3 * 4 * 20 + 2 * 3 * 5 * 4
    assert L.piml_crowd_stats_voronoi_workspace_bytes(2, 3, 5, 4) == L.piml_crowd_stats_workspace_bytes(2, 3, 4) + 120
    assert L.piml_crowd_stats_voronoi_workspace_bytes(1, 1, -1, 1) == -1
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)
    dirs = (ctypes.c_float * 64)(*([1.0, 0.0] * 32))

    def call(S=1, T=2, N=3, t0=0, t1=2, cutoff=1.0, dirs=ctypes.addressof(dirs), sides=16, hb=0, bx0=0., bx1=1., by0=0.,
             by1=1., box=0, x0=0., x1=1., y0=0., y1=1., h=0.5, gx=2, gy=2, rb=0.25, B=4, P=q, n=q, mp=q, dropped=q, ws=q,
             wsb=1 << 20):
        return L.piml_crowd_stats_voronoi(P, q, q, None, S, T, N, t0, t1, cutoff, dirs, sides, hb, bx0, bx1, by0, by1, box,
                                          x0, x1, y0, y1, h, gx, gy, rb, B, n, q, q, q, q, q, q, mp, None, dropped, ws, wsb,
                                          None)
    nan, inf = float('nan'), float('inf')
    for bad in (dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=nan), dict(cutoff=inf), dict(sides=2), dict(sides=33),
                dict(dirs=None), dict(dropped=None), dict(hb=1, bx1=0.0), dict(hb=1, by0=1.0), dict(hb=1, bx0=nan),
                dict(hb=1, by1=inf),
                # what piml_crowd_stats refuses
                dict(S=0), dict(T=0), dict(N=-1), dict(B=0), dict(B=257), dict(rb=0.0), dict(t0=1, t1=1), dict(t1=3),
                dict(t0=-1), dict(box=1, x1=0.), dict(box=1, y0=2.), dict(box=1, h=0.), dict(box=1, gx=0),
                dict(box=1, mp=None), dict(P=None), dict(n=None), dict(ws=None), dict(wsb=2 * 4 * 20 + 2 * 3 * 4 - 1)):
        assert call(**bad) == 1, bad
