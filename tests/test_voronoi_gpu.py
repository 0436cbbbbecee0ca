"""GPU: the Voronoi density of the crowd statistics (piml_crowd_stats_voronoi) against closed forms, the
partition property and the numpy restatement of the cell (voronoi_ref.py, float64 and float32) on random slices and the
recorded GC and UCY clips; vertex growth up to and past the polygon's capacity; determinism (two calls, graph replay,
member against a one-member call, an ensemble against its members); the Gaussian path around a Voronoi call."""
import math
import os

import numpy as np
import pytest
import torch

import crowdstats_ref as REF
import voronoi_ref as VREF
from conftest import GOLDEN
from test_crowdstats_gpu import FD, GC_BOX, GC_CLIP, SERIES, random_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UCY_CLIP = 'UCY_Dataset_time162-216_timeunit0.08'
NAMES = SERIES + FD + ('map', 'dropped')
TILE = 1024                                  # CD_TILE: the present agents one LDS tile holds


def voronoi(P, M, V=None, **kw):
    from piml_amd.crowdstats import crowd_stats
    V = np.zeros_like(P) if V is None else V
    return crowd_stats(torch.tensor(P, device=DEV), torch.tensor(V, device=DEV), torch.tensor(M, device=DEV),
                       density='voronoi', return_density=True, **kw)


def one_slice(points, **kw):
    """The device's areas (1 / rho, float64) and dropped count of one slice of present agents."""
    P = np.asarray(points, np.float32)[None]
    st = voronoi(P, np.ones(P.shape[:2], np.float32), **kw)
    return 1.0 / st.density[0, 0].astype(np.float64), int(st.dropped[0]), st


def dirs(sides=16):
    from piml_amd.crowdstats import voronoi_dirs
    return voronoi_dirs(sides)


def test_closed_forms():
    """1e-5 relative, the project's parity bar."""
    for sides, cutoff in ((16, 1.0), (3, 0.7), (32, 2.5), (5, 1e3)):
        area, dropped, st = one_slice([[3.25, -7.5]], cutoff=cutoff, sides=sides)
        c = float(np.float32(cutoff))
        want = sides / 2 * c * c * math.sin(2 * math.pi / sides)
        assert abs(area[0] - want) <= 1e-5 * want and dropped == 0, (sides, cutoff)
        assert st.n.tolist() == [[1]] and st.sum_density[0, 0] == float(st.density[0, 0, 0])
    # two agents 0.8 apart: halves of the union of their cut-off polygons
    pts = np.float32([[1.0, 2.0], [1.0 + 0.8 * math.cos(0.3), 2.0 + 0.8 * math.sin(0.3)]])
    area, dropped, _ = one_slice(pts, cutoff=1.0)
    want, _, _ = VREF.cells(pts, np.ones(2), 1.0, dirs())
    assert abs(area[0] - area[1]) <= 1e-5 * area[0] and abs(area.sum() - want.sum()) <= 1e-5 * want.sum() and dropped == 0
    assert area[0] < 0.9 * 8 * math.sin(math.pi / 8)                # (each was cut)
    # a 2 x 2 lattice inside the bounds, no cut-off to speak of: a quarter each
    pts = np.float32([[10, 20], [20, 20], [10, 30], [20, 30]])
    area, dropped, _ = one_slice(pts, cutoff=1e3, bounds=GC_BOX)
    assert np.abs(area - 100.0).max() <= 1e-5 * 100.0 and dropped == 0
    # coincident agents share the unclipped cell
    area, dropped, _ = one_slice([[4.0, 4.0], [4.0, 4.0]], cutoff=1.0)
    assert np.abs(area - 8 * math.sin(math.pi / 8)).max() <= 1e-5 * 8 * math.sin(math.pi / 8) and dropped == 0


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257, TILE + 1])
def test_partition_on_the_device(n):
    """n agents uniform in the bounds, cutoff 1e3: the cells tile the bounds.  The bound is 4 x the partition error of the
    restatement's float32 run on the same slice (so a different summation order is covered).  Measured, the float32 run's
    relative error: 7.28e-8 (n = 1), 4.07e-9 (2), 2.34e-8 (63), 8.32e-9 (64), 2.09e-8 (65), 6.11e-9 (257), 1.07e-8 (1025),
    and the device's (MI355X) the same to the three digits shown: the device's float32 geometry is the restatement's,
    operation for operation, and what is left is the float32 rounding of each area and of its reciprocal."""
    rng = np.random.default_rng(n)
    side = math.sqrt(n / 1.5)
    bounds = (1.0, 1.0 + side, -2.0, -2.0 + side)
    pts = (rng.random((n, 2)) * side * 0.999 + np.float64([1.0, -2.0])).astype(np.float32)
    want = (float(np.float32(bounds[1])) - 1.0) * (float(np.float32(bounds[3])) + 2.0)
    a32, _, peak = VREF.cells(pts, np.ones(n), 1e3, dirs(), bounds=bounds, dtype=np.float32)
    err32 = abs((1.0 / VREF.rho_of(a32).astype(np.float64)).sum() - want) / want
    area, dropped, st = one_slice(pts, cutoff=1e3, bounds=bounds)
    err = abs(area.sum() - want) / want
    print(f'n = {n}: partition error float32 restatement {err32:.3g}, device {err:.3g}')
    assert dropped == 0 and st.n.tolist() == [[n]] and peak.max() <= 64
    assert err32 < 1e-6 and err <= 4 * err32


def check_against_restatement(st, P, V, M, cutoff, n_active=None, max_left_out=0.01, **kw):
    """Focal sets and NaN patterns equal; areas within 1e-5 of the float64 restatement except where its own float32 run
    misses 1e-5 (at most 1 % of the focal cells); everything downstream exact given the device's densities."""
    S, T = M.shape[:2]
    a, b = kw.get('frames') or (0, T)
    geo = dict(bounds=kw.get('bounds'), box=kw.get('box'))
    focal = left_out = 0
    for s in range(S):
        na = None if n_active is None else n_active[s]
        a64, _, peak = VREF.cells_frames(P[s, a:b], M[s, a:b], cutoff, dirs(), n_active=na, **geo)
        a32, _, _ = VREF.cells_frames(P[s, a:b], M[s, a:b], cutoff, dirs(), n_active=na, dtype=np.float32, **geo)
        assert peak.max() <= 64
        got = st.density[s]
        assert np.array_equal(np.isnan(got), np.isnan(a64)), s
        ok = ~np.isnan(a64)
        rel = np.abs(1.0 / got[ok].astype(np.float64) - a64[ok]) / a64[ok]
        slivers = np.abs(a32[ok] - a64[ok]) > 1e-5 * a64[ok]
        assert (rel[~slivers] <= 1e-5).all(), (s, rel[~slivers].max())
        focal, left_out = focal + int(ok.sum()), left_out + int(slivers.sum())
    assert focal > 0 and left_out <= max_left_out * focal, (left_out, focal)
    assert st.dropped.tolist() == [0] * S
    # downstream of the densities: the Gaussian restatement's sums, over the agents that have a density
    Mx = np.array(M, np.float32)
    Mx[:, a:b][np.isnan(st.density)] = 0.0
    ref_kw = {k: v for k, v in kw.items() if k in ('box', 'cell', 'rho_bin', 'rho_bins', 'frames')}
    exact = REF.crowd_stats(P, V, Mx, n_active=n_active, rho=st.density, **ref_kw)
    for k in ('n', 'n_speed', 'fd_count'):
        assert np.array_equal(getattr(st, k), exact[k]), k
    for k in ('sum_speed', 'sum_density', 'fd_sum', 'fd_sum2'):
        np.testing.assert_allclose(getattr(st, k), exact[k], rtol=1e-12, atol=1e-300, err_msg=k)
    assert (st.map is None) if kw.get('box') is None else np.array_equal(st.map, exact['map'])
    return focal, left_out


@pytest.mark.parametrize('seed', [1, 2])
def test_random_slices_against_the_restatement(seed):
    """Absent slots, NaN / infinite positions, masks that are neither 0 nor 1, non-finite velocities, agents outside the box
    and outside the bounds, n_active below N.  Seeds 1 and 2, measured on the CPU: the float32 restatement misses 1e-5 on
    0 of 440 / 432 focal cells (largest relative error 4e-7), so no cell is left out."""
    S, T, N = 2, 3, 300
    P, V, M, side = random_slices(S, T, N, seed)
    n_active = [N, N - 40]
    kw = dict(box=(0.0, 0.55 * side, 0.1 * side, 0.7 * side), bounds=(-0.1 * side, 0.6 * side, 0.0, 0.75 * side), cell=0.37,
              rho_bin=0.2, rho_bins=9)
    st = voronoi(P, M, V, cutoff=1.0, n_active=n_active, **kw)
    focal, left_out = check_against_restatement(st, P, V, M, 1.0, n_active=n_active, **kw)
    assert focal > 300 and left_out == 0 and (st.fd_count > 0).sum() >= 4
    st = voronoi(P, M, V, cutoff=0.6, frames=(1, 3))                # no box, no bounds, a frame range, another cut-off
    check_against_restatement(st, P, V, M, 0.6, frames=(1, 3))
    assert st.options['density'] == 'voronoi' and st.options['cutoff'] == 0.6 and st.options['sides'] == 16


def _raw(name):
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(os.path.join(GOLDEN, 'data', name + '.npy'))
    return raw


@pytest.mark.parametrize('name,box', [(GC_CLIP, GC_BOX), (UCY_CLIP, None)])
def test_recorded_clips_against_the_restatement(name, box):
    """Frames 300 .. 349, cutoff 1.0 (GC: the box is also the walkable area).  Measured on the CPU: the float32 restatement
    misses 1e-5 on 0 of the 1290 (GC) / 1008 (UCY) focal cells, largest relative error 2e-7."""
    from piml_amd.crowdstats import crowd_stats_of_raw
    raw = _raw(name)
    P, V, M = (x.numpy()[None] for x in (raw.position, raw.velocity, raw.mask_p))
    kw = dict(frames=(300, 350)) if box is None else dict(frames=(300, 350), box=box, bounds=box)
    st = crowd_stats_of_raw(raw, density='voronoi', cutoff=1.0, return_density=True, **kw)
    focal, left_out = check_against_restatement(st, P, V, M, 1.0, **kw)
    assert focal > 900 and left_out == 0 and st.n.shape == (1, 50)


def _ring(m, radius=1.97, phase=0.1):
    ang = phase + 2 * np.pi * np.arange(m) / m
    ring = radius * np.stack([np.cos(ang), np.sin(ang)], 1)
    return (np.concatenate([[[0.0, 0.0]], ring]) + [3.0, -2.0]).astype(np.float32)


def test_vertex_growth_and_capacity():
    """A focal agent whose neighbours stand on a ring just inside 2 cutoff: every bisector shaves a corner.  The neighbour
    counts come from the restatement: the first whose polygon ends with more than 32 and fewer than 64 vertices, one that
    ends with exactly 64 if there is one, and the first that passes 64 on the way."""
    d, grows, full, over = dirs(), None, None, None
    for m in range(20, 100, 2):
        pts = _ring(m)
        area, verts, peak = VREF.cells(pts, np.ones(m + 1), 1.0, d)
        if grows is None and 32 < verts[0] < 64 and peak[0] < 64:
            grows = (pts, area)
        if full is None and peak[0] == 64:
            full = (pts, area)
        if peak[0] > 64:
            over = (pts, area)
            break
    assert grows is not None and over is not None
    for pts, want in filter(None, (grows, full)):
        area, dropped, st = one_slice(pts, cutoff=1.0)
        assert dropped == 0 and np.abs(area - want).max() <= 1e-5 * want.min() and st.n.tolist() == [[len(pts)]]
    pts, want = over
    V = np.ones((1, len(pts), 2), np.float32)
    st = voronoi(pts[None], np.ones((1, len(pts)), np.float32), V, cutoff=1.0)
    rho = st.density[0, 0]
    assert np.isnan(rho[0]) and not np.isnan(rho[1:]).any() and st.dropped.tolist() == [1]
    assert st.n.tolist() == [[len(pts) - 1]] and st.n_speed.tolist() == [[len(pts) - 1]]
    assert st.fd_count.sum() == len(pts) - 1
    assert (np.abs(1.0 / rho[1:].astype(np.float64) - want[1:]) <= 1e-5 * want[1:]).all()
    assert st.sum_density[0, 0] == pytest.approx(rho[1:].astype(np.float64).sum(), rel=1e-12)
    # the same neighbours without the agent in the middle: their cells on the inner side differ, their count does not
    rest = voronoi(pts[None, 1:], np.ones((1, len(pts) - 1), np.float32), V[:, 1:], cutoff=1.0)
    assert rest.dropped.tolist() == [0] and rest.n.tolist() == st.n.tolist()


def _bits(x):
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.int64) if x.dtype == np.float64 else x


def _same(a, b, names=NAMES + ('slices', 'density')):
    return [k for k in names if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]


def test_determinism_graph_and_members():
    from piml_amd import ops_metrics
    from piml_amd.crowdstats import crowd_stats, voronoi_dirs
    S, T, N = 3, 20, 300
    P, V, M, side = random_slices(S, T, N, seed=7)
    Pt, Vt, Mt = (torch.tensor(x, device=DEV) for x in (P, V, M))
    rect = (0.0, side * 0.6, 0.0, side * 0.6)
    kw = dict(box=rect, bounds=rect, cell=0.5, density='voronoi', cutoff=1.0, return_density=True)
    n_active = [N, N - 37, N - 150]
    a, b = crowd_stats(Pt, Vt, Mt, n_active=n_active, **kw), crowd_stats(Pt, Vt, Mt, n_active=n_active, **kw)
    assert not _same(a, b) and a.n.sum() > 1000
    for m in range(S):                       # member m of the S-member call == an S = 1 call on member m
        one = crowd_stats(Pt[m], Vt[m], Mt[m], n_active=[n_active[m]], **kw)
        assert not _same(a.member(m), one), m
    grid = (a.map.shape[2], a.map.shape[1])
    na = torch.tensor(n_active, device=DEV, dtype=torch.int32)
    args = (Pt, Vt, Mt, 1.0, voronoi_dirs(16), rect, rect, grid, 0.5, 0.25, 24, (0, T), True, na)
    eager = ops_metrics.crowd_stats_voronoi_frames(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops_metrics.crowd_stats_voronoi_frames(*args)            # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops_metrics.crowd_stats_voronoi_frames(*args)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(cap[k].cpu().numpy())), k
    assert np.array_equal(eager['n'].cpu().numpy(), a.n) and np.array_equal(eager['dropped'].cpu().numpy(), a.dropped)


def test_ensemble_against_its_members():
    """ScenarioEnsemble.crowd_stats(density='voronoi') of an MLAPM-driven GC ensemble: member m is bitwise the one-member
    call and the statistics of the member written out as a clip, the simulated velocities kept."""
    from piml_amd.crowdstats import crowd_stats_of_raw
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to(DEV)
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    ens = law.simulate_ensemble(sc, 40, [0, 1, 2])
    kw = dict(density='voronoi', box=GC_BOX, bounds=GC_BOX)
    st = ens.crowd_stats(**kw)
    assert st.n.shape == (3, 40) and st.n.sum() > 0 and st.options['density'] == 'voronoi'
    names = NAMES + ('slices',)
    for m in range(3):
        mem = ens.member(m)
        assert not _same(st.member(m), mem.crowd_stats(**kw), names), m
        assert not _same(st.member(m), crowd_stats_of_raw(mem.to_raw_data(), **kw), names), m


def test_the_gaussian_path_is_untouched():
    """The same Gaussian call before and after a Voronoi call on the same tensors: the shared statistics pass and the
    allocator's reuse of the workspace leave it bitwise what it was."""
    from piml_amd.crowdstats import crowd_stats
    P, V, M, side = random_slices(2, 6, 300, seed=11)
    Pt, Vt, Mt = (torch.tensor(x, device=DEV) for x in (P, V, M))
    kw = dict(box=(0.0, side * 0.6, 0.0, side * 0.6), cell=0.5, return_density=True)
    before = crowd_stats(Pt, Vt, Mt, **kw)
    vor = crowd_stats(Pt, Vt, Mt, density='voronoi', bounds=kw['box'], **kw)
    after = crowd_stats(Pt, Vt, Mt, **kw)
    assert not _same(before, after) and before.options == after.options and before.options['density'] == 'gaussian'
    assert before.dropped.tolist() == [0, 0] and _same(before, vor, ('sum_density', 'density'))
    assert np.array_equal(before.n >= vor.n, np.ones_like(before.n, bool))
