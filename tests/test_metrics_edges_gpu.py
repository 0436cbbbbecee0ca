"""GPU: the Sinkhorn OT and MMD kernels (piml_amd/csrc/metrics.hip) outside the region test_metrics_hip_gpu.py covers, on
the frames of metrics_edges_shapes.py: masked frames of more than one 1024-slot chunk, different masks and slot counts
on the two sides, eps and thresh other than 0.1, a few present points among thousands of slots, empty sides.  Against the
reference's recorded values (tests/golden/metrics_edges.npz), the float64 restatement (sinkhorn64), the same points
compacted on the host, and closed forms.  Every kernel result is computed once per process and shared."""
import functools

import numpy as np
import pytest
import torch

import metrics_edges_shapes as SH
from conftest import bits, golden
from test_metrics_hip_gpu import mmd64

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SETS = ('chunks', 'sparse', 'small')


def on_gpu(name):
    x, mx, y, my = SH.frames(name) if isinstance(name, str) else name
    return x.to(DEV), y.to(DEV), mx.to(DEV), my.to(DEV)                   # the operators' argument order


@functools.lru_cache(maxsize=None)
def masked(name, eps=0.1, thresh=SH.REF_THRESH, max_iter=100):
    """the masked call on a whole set: cost (F), iters (F), u (F, n), v (F, m) as numpy"""
    from piml_amd import ops_metrics
    out = ops_metrics.sinkhorn_frames(*on_gpu(name), eps=eps, thresh=thresh, max_iter=max_iter, want_potentials=True)
    cost, iters, u, v = (t.cpu().numpy() for t in out)
    return cost, iters, u, v


@functools.lru_cache(maxsize=None)
def compact_call(name, f, eps=0.1, thresh=SH.REF_THRESH, max_iter=100):
    """frame f's present points, compacted on the host, without masks"""
    from piml_amd import ops_metrics
    x, y = SH.compacted(name, f)
    out = ops_metrics.sinkhorn_frames(x[None].to(DEV), y[None].to(DEV), eps=eps, thresh=thresh, max_iter=max_iter,
                                      want_potentials=True)
    cost, iters, u, v = (t.cpu().numpy()[0] for t in out)
    return cost, iters, u, v


@functools.lru_cache(maxsize=None)
def mmd_masked(name):
    from piml_amd import ops_metrics
    return ops_metrics.mmd_frames(*on_gpu(name)).cpu().numpy()


def present(name):
    _, mx, _, my = SH.frames(name)
    return mx.numpy() == 1, my.numpy() == 1


# ----------------------------------------------------------------------------------------------------------------------
# 1. cost and iteration count per frame
@pytest.mark.parametrize('name,eps,thresh', SH.GROUPS)
def test_cost_and_iterations_per_frame(name, eps, thresh):
    """Iterations equal the float64 restatement's.  Cost: thresh 0.1 against the reference's recorded float32 value within
    the group's tolerance (3 x the reference's own float32-vs-float64 spread, 1e-5 at the least; measured: 1e-5 for every
    group but sparse at eps 0.01, 1.06e-3, and at eps 0.1, 4.9e-5).  The frame the reference cannot run (one y point), and
    every (eps, thresh) with another thresh, against the float64 restatement, the bound made likewise from the float32
    restatement's spread."""
    g = golden('metrics_edges')
    cost, iters, _, _ = masked(name, eps, thresh)
    ref = SH.ref64(name, eps, thresh)
    band = SH.band_frames(name, eps, thresh)
    recorded = thresh == SH.REF_THRESH
    tol = SH.cost_tolerance(g, name, eps) if recorded else SH.restated_cost_tolerance(name, eps, thresh)
    rows = []
    for f, (want64, it64, _, _, _) in enumerate(ref):
        want = g[f'{name}/ot32_{eps}'][f] if recorded else want64
        if np.isnan(want):
            want = want64
        rows.append((f, int(iters[f]), it64, float(cost[f]), want, abs(float(cost[f]) - want) / abs(want)))
    print(f'\n{name} eps {eps} thresh {thresh}: tolerance {tol:.2e}, {len(band)} of {len(ref)} frames in the band')
    for r in rows:
        print('  frame %d iterations %d (float64 %d) cost %.9g want %.9g rel %.2e' % r)
    assert len(band) <= 0.02 * len(ref)
    for f, it, it64, c, want, rel in rows:
        if f in band:
            assert abs(it - it64) <= 1, (name, eps, thresh, f, it, it64)
            continue
        assert it == it64, (name, eps, thresh, f, it, it64)
        assert rel <= tol, (name, eps, thresh, f, c, want, rel, tol)


# ----------------------------------------------------------------------------------------------------------------------
# 2. masked equals compacted
def test_dense1k_masked_equals_compacted_bit_for_bit():
    """Both calls run 16 waves over the same compacted order: cost, iters, u, v at present slots and MMD carry the same
    bits; u, v are exactly 0 at absent slots."""
    from piml_amd import ops_metrics
    x, mx, y, my = SH.frames('dense1k')
    cost, iters, u, v = masked('dense1k', max_iter=10)
    px, py = present('dense1k')
    cx = torch.stack([x[f][mx[f] == 1] for f in range(x.shape[0])]).to(DEV)
    cy = torch.stack([y[f][my[f] == 1] for f in range(y.shape[0])]).to(DEV)
    assert cx.shape == (2, 1100, 2) and cy.shape == (2, 1000, 2)
    c2, i2, u2, v2 = (t.cpu().numpy() for t in ops_metrics.sinkhorn_frames(cx, cy, max_iter=10, want_potentials=True))
    assert (iters == 10).all() and (i2 == 10).all()
    assert np.array_equal(bits(cost), bits(c2))
    for f in range(2):
        assert np.array_equal(bits(u[f][px[f]]), bits(u2[f])) and np.array_equal(bits(v[f][py[f]]), bits(v2[f])), f
        assert np.array_equal(bits(u[f][~px[f]]), np.zeros((~px[f]).sum(), np.uint32))
        assert np.array_equal(bits(v[f][~py[f]]), np.zeros((~py[f]).sum(), np.uint32))
    assert np.isfinite(cost).all() and (cost > 0).all() and np.abs(u).max() > 0
    assert np.array_equal(bits(mmd_masked('dense1k')), bits(ops_metrics.mmd_frames(cx, cy).cpu().numpy()))


@pytest.mark.parametrize('name,eps', [('chunks', 0.1), ('chunks', 0.01), ('sparse', 0.1), ('sparse', 1.0)])
def test_masked_against_compacted_with_other_wave_counts(name, eps):
    """The compacted call runs fewer waves.  Each row's log-sum-exp is one wave's work whatever the wave count, so u, v
    carry the same bits whenever the iteration counts agree (they may differ only in the band); the cost's float64 sum
    runs in another order: within 2 float32 ulp."""
    cost, iters, u, v = masked(name, eps)
    px, py = present(name)
    band = SH.band_frames(name, eps)
    for f in range(SH.n_frames(name)):
        c2, i2, u2, v2 = compact_call(name, f, eps)
        assert f in band or iters[f] == i2, (name, f, iters[f], i2)
        assert (u[f][~px[f]] == 0).all() and (v[f][~py[f]] == 0).all()
        if iters[f] == i2:
            assert np.array_equal(bits(u[f][px[f]]), bits(u2)) and np.array_equal(bits(v[f][py[f]]), bits(v2)), (name, f)
            assert abs(float(cost[f]) - float(c2)) <= 2 * float(np.spacing(np.float32(abs(c2)))), (name, f, cost[f], c2)


@pytest.mark.parametrize('name', ['chunks', 'sparse'])
def test_mmd_masked_against_compacted(name):
    from piml_amd import ops_metrics
    out = mmd_masked(name).astype(np.float64)
    for f in range(SH.n_frames(name)):
        x, y = SH.compacted(name, f)
        want = float(ops_metrics.mmd_frames(x[None].to(DEV), y[None].to(DEV))[0])
        assert abs(out[f] - want) <= 1e-12 * abs(want), (name, f, out[f], want)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the potentials' values
@pytest.mark.parametrize('name', ['chunks', 'small'])
def test_potentials_against_float64(name):
    """u, v at present slots against sinkhorn64's, within 3 x the float32 restatement's largest |u32 - u64| in the group
    (measured: chunks 2.7e-5, small 2.2e-5).  The column marginals are exact after the v half-step: sum_i exp(M_ij), formed
    in float64 from the returned u, v, equals 1/m + 1e-8 within that tolerance / eps, relative."""
    eps = 0.1
    tol, _ = SH.potential_tolerance(name, eps)
    cost, iters, u, v = masked(name, eps)
    px, py = present(name)
    band = SH.band_frames(name, eps)
    rows = []
    for f, (_, it64, _, u64, v64) in enumerate(SH.ref64(name, eps)):
        if f in band:
            continue
        x, y = SH.compacted(name, f)
        uf, vf = torch.tensor(u[f][px[f]]).double(), torch.tensor(v[f][py[f]]).double()
        C = ((x.double().unsqueeze(1) - y.double().unsqueeze(0)) ** 2).sum(-1)
        col = torch.exp((-C + uf.unsqueeze(1) + vf.unsqueeze(0)) / eps).sum(0)
        nu = 1.0 / y.shape[0] + 1e-8
        rows.append((f, int(iters[f]), it64, float((uf - u64).abs().max()), float((vf - v64).abs().max()),
                     float((col / nu - 1).abs().max())))
    print(f'\n{name}: potentials within {tol:.2e}, marginals within {tol / eps:.2e}')
    for r in rows:
        print('  frame %d iterations %d (float64 %d) |u - u64| %.2e |v - v64| %.2e marginal %.2e' % r)
    assert rows
    for f, it, it64, du, dv, dm in rows:
        assert it == it64 and du <= tol and dv <= tol and dm <= tol / eps, (name, f, it, it64, du, dv, dm, tol)


# ----------------------------------------------------------------------------------------------------------------------
# 4. closed forms
@pytest.mark.parametrize('eps', [0.1, 0.01])
def test_perm_lattice_cost_is_the_matching(eps):
    """The optimal plan is the matching and its blur is of order exp(-22 / eps): cost = |d|^2 (1 + 1521e-8) within 1e-5
    after 2 iterations, whatever the slot order of x."""
    want = SH.perm_cost()
    cost, iters, u, v = masked('perm', eps)
    c2, i2, _, _ = masked('perm_relabelled', eps)
    print(f'\nperm eps {eps}: cost {cost[0]!r} relabelled {c2[0]!r} want {want!r}, iterations {iters[0]} / {i2[0]}')
    assert iters[0] == 2 and i2[0] == 2
    assert abs(float(cost[0]) - want) <= 1e-5 * want and abs(float(c2[0]) - want) <= 1e-5 * want
    assert abs(float(cost[0]) - float(c2[0])) <= 1e-6 * want
    px, py = present('perm')
    assert (u[0][~px[0]] == 0).all() and (v[0][~py[0]] == 0).all() and np.isfinite(u).all() and np.isfinite(v).all()


@pytest.mark.parametrize('eps', [0.1, 1.0])
def test_one_point_against_many_is_the_forced_plan(eps):
    """sparse's frames 2 (1 against 500) and 3 (500 against 1): cost = the forced plan's, in float64, within 1e-5.  Not at
    eps 0.01, where the float32 restatement itself sits 2e-4 from it (v_j ~ C_j carries ulp(C) / eps of relative error)."""
    cost = masked('sparse', eps)[0]
    for f in (2, 3):
        want = SH.one_against_many(*SH.compacted('sparse', f))
        print(f'\nsparse frame {f} eps {eps}: cost {cost[f]!r} want {want!r} rel {abs(float(cost[f]) - want) / want:.2e}')
        assert abs(float(cost[f]) - want) <= 1e-5 * want, (f, eps, cost[f], want)


# ----------------------------------------------------------------------------------------------------------------------
# 5. empty and single-point sides
def test_degenerate_frames_return_the_documented_values_and_leave_their_neighbours_alone():
    """What include/piml_hip.h documents for a frame with an empty side or one point a side, and that sparse's frames
    between them carry the bits of a call without them."""
    from piml_amd import ops_metrics
    sets = SH.degenerate()
    keep = sets[4]
    x, y, mx, my = on_gpu(sets[:4])
    cost, iters, u, v = (t.cpu().numpy() for t in ops_metrics.sinkhorn_frames(x, y, mx, my, want_potentials=True))
    mmd = ops_metrics.mmd_frames(x, y, mx, my).cpu().numpy()
    for got, want in zip((cost, iters, u, v), masked('sparse')):
        assert np.array_equal(got[keep].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bits(mmd[keep]), bits(mmd_masked('sparse')))
    px, py = sets[1].numpy() == 1, sets[3].numpy() == 1
    inf = np.float32(np.inf)
    # x empty (frame 1), both empty (frame 5): err = 0 stops the loop after one iteration; v = +inf where y is present
    assert cost[1] == 0 and iters[1] == 1 and (u[1] == 0).all() and (v[1][py[1]] == inf).all() and (v[1][~py[1]] == 0).all()
    assert cost[5] == 0 and iters[5] == 1 and (u[5] == 0).all() and (v[5] == 0).all()
    # y empty (frame 3): err is inf, then NaN: every iteration runs; u = +inf where x is present
    assert cost[3] == 0 and iters[3] == 100 and (u[3][px[3]] == inf).all() and (u[3][~px[3]] == 0).all() and (v[3] == 0).all()
    c7, i7, u7, v7 = (t.cpu().numpy() for t in ops_metrics.sinkhorn_frames(x, y, mx, my, max_iter=7, want_potentials=True))
    assert i7[3] == 7 and i7[1] == 1 and i7[5] == 1 and c7[3] == 0
    c0, i0, u0, v0 = (t.cpu().numpy() for t in ops_metrics.sinkhorn_frames(x, y, mx, my, max_iter=0, want_potentials=True))
    assert (i0 == 0).all() and (u0 == 0).all() and (v0 == 0).all() and c0[1] == c0[3] == c0[5] == 0
    # one point a side (frame 7): the squared distance after 2 iterations, u + v = it
    a, b = sets[0][7][px[7]].double(), sets[2][7][py[7]].double()
    d2 = float(((a - b) ** 2).sum())
    assert iters[7] == 2 and abs(float(cost[7]) - d2) <= 1e-5 * d2, (cost[7], d2)
    assert abs(float(u[7][px[7]][0]) + float(v[7][py[7]][0]) - d2) <= 1e-5 * d2
    # MMD: an empty block adds 0
    assert abs(float(mmd[1]) - mmd_block(sets[2][1][py[1]])) <= 1e-5 * abs(float(mmd[1])) and mmd[1] > 0
    assert abs(float(mmd[3]) - mmd_block(sets[0][3][px[3]])) <= 1e-5 * abs(float(mmd[3])) and mmd[3] > 0
    assert mmd[5] == 0                                                               # no point at all: every block is empty
    want = mmd64(a, b)
    assert abs(float(mmd[7]) - want) <= max(1e-5 * abs(want), 1e-9)
    # one point in total: N^2 - N == 0, the bandwidth and the result are NaN
    none = torch.zeros_like(my[7:8])
    assert np.isnan(float(ops_metrics.mmd_frames(x[7:8], y[7:8], mx[7:8], none)[0]))
    assert np.isnan(float(ops_metrics.mmd_frames(x[7:8], y[7:8], none, my[7:8])[0]))


def mmd_block(p, kernel_mul=2.0, kernel_num=5):
    """the XX / n^2 (or YY / m^2) term of a frame whose other side is empty, float64, written out here"""
    p = p.double()
    k = p.shape[0]
    L2 = ((p.unsqueeze(0) - p.unsqueeze(1)) ** 2).sum(-1)
    bw = L2.sum() / (k * k - k) / kernel_mul ** (kernel_num // 2)
    return float(sum(torch.exp(-L2 / (bw * kernel_mul ** i)) for i in range(kernel_num)).sum() / (k * k))


@pytest.mark.parametrize('name', SETS)
def test_mmd_with_different_masks_against_float64(name):
    """mask_x != mask_y, n != m: against _mmd_torch in float64 on the compacted points within max(1e-5 |want|, 1e-9), and
    against the reference's recorded float32 value within 3 x its own float32-vs-float64 spread."""
    g = golden('metrics_edges')
    out = mmd_masked(name).astype(np.float64)
    for f in range(SH.n_frames(name)):
        want = mmd64(*SH.compacted(name, f))
        r32, r64 = g[f'{name}/mmd32'][f], g[f'{name}/mmd64'][f]
        print(f'\n{name} frame {f}: mmd {out[f]!r} float64 {want!r} reference {r32!r} / {r64!r}')
        assert abs(out[f] - want) <= max(1e-5 * abs(want), 1e-9), (name, f, out[f], want)
        assert abs(out[f] - r32) <= max(3 * abs(r32 - r64), 1e-8), (name, f, out[f], r32, r64)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the functions layer
@pytest.mark.parametrize('eps', [0.01, 1.0])
def test_ot_with_time_mask_passes_eps_on(eps):
    """impl='hip' against impl='torch' per frame on a (T, 2500, 2) masked input, within chunks' tolerance at that eps"""
    from piml_amd.functions import metrics as M
    p, q, mask = (t.to(DEV) for t in SH.functions_input())
    tol = SH.cost_tolerance(golden('metrics_edges'), 'chunks', eps)
    hip = M.ot_with_time_mask(p, q, mask, eps=eps, impl='hip')
    tor = M.ot_with_time_mask(p, q, mask, eps=eps, impl='torch')
    print(f'\not_with_time_mask eps {eps}: hip {hip} torch {tor} tolerance {tol:.2e}')
    assert len(hip) == len(tor) == p.shape[0]
    for f, (a, b) in enumerate(zip(hip, tor)):
        assert abs(a - b) <= tol * abs(b), (eps, f, a, b)
    assert abs(M.ot_with_time_mask(p, q, mask, eps=eps, reduction='mean', impl='hip') - np.mean(tor)) <= tol * np.mean(tor)


def test_wasserstein_distance_2d_small_eps_gpu_against_cpu():
    from piml_amd.functions import metrics as M
    x, y = SH.compacted('chunks', 0)
    tol = SH.cost_tolerance(golden('metrics_edges'), 'chunks', 0.01)
    dist, P, C = M.wasserstein_distance_2d(x.to(DEV), y.to(DEV), eps=0.01)
    want, Pw, Cw = M.wasserstein_distance_2d(x, y, eps=0.01)
    print(f'\nwasserstein_distance_2d eps 0.01: gpu {float(dist)!r} cpu {float(want)!r}')
    assert dist.is_cuda and P.shape == (300, 200)
    assert abs(float(dist) - float(want)) <= tol * float(want)
    assert np.allclose(C.cpu().numpy(), Cw.numpy(), rtol=1e-6, atol=0)
    # P is formed from the kernel's u, v: its cost is the kernel's, its column sums are nu
    assert abs(float((P.double() * C.double()).sum()) - float(dist)) <= 1e-5 * float(dist)
    assert np.allclose(P.double().sum(0).cpu().numpy(), 1.0 / 200 + 1e-8, rtol=1e-3, atol=0)
