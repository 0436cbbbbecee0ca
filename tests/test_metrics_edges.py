"""CPU-only: the preconditions of test_metrics_edges_gpu.py.  The frames of metrics_edges_shapes.py really leave the region
the older fixtures cover (more slots than the kernels' thread cap, the mask patterns their docstring lists, 1024 threads
for dense1k masked and compacted), no frame's float64 err passes within 1e-4 of its threshold, the values recorded in
tests/golden/metrics_edges.npz agree with the float64 restatement within their own spread, and the closed forms the GPU
tests assert hold for the float64 restatement."""
import numpy as np
import pytest
import torch

import metrics_edges_shapes as SH
from conftest import golden
from test_metrics_hip_gpu import BAND, THRESH, mmd64, sinkhorn64


def test_slot_counts_exceed_the_thread_cap_and_dense1k_takes_it_in_both_forms():
    lo, cap = SH.thread_limits()
    assert cap == SH.CHUNK and SH.WAVE == 64 and lo == 256
    for name in ('chunks', 'sparse', 'dense1k', 'perm'):
        x, mx, y, my = SH.frames(name)
        assert x.shape[1] > cap and y.shape[1] > cap, name
        assert x.shape[1] >= y.shape[1]
    x, mx, y, my = SH.frames('sparse')
    assert x.shape[1] == 2 * cap
    x, mx, y, my = SH.frames('dense1k')
    assert mx.sum(-1).tolist() == [1100, 1100] and my.sum(-1).tolist() == [1000, 1000]
    assert SH.metric_threads(x.shape[1], y.shape[1]) == cap == SH.metric_threads(1100, 1000)
    # chunks and sparse: the compacted call runs fewer waves than the masked one
    assert SH.metric_threads(300, 200) < cap and SH.metric_threads(3, 5) == lo
    x, mx, y, my = SH.frames('small')
    assert x.shape[1:] == (65, 2) and y.shape[1:] == (64, 2) and bool(mx.all()) and bool(my.all())
    assert SH.metric_threads(65, 64) == lo and 65 > lo // 64 * (64 // 4)          # 4 waves, 16 whole rounds of rows, + 1 row


def test_every_set_holds_nan_exactly_at_absent_slots():
    for name in ('chunks', 'sparse', 'small', 'dense1k', 'perm', 'perm_relabelled'):
        x, mx, y, my = SH.frames(name)
        for p, m in ((x, mx), (y, my)):
            assert p.dtype == torch.float32 and set(m.unique().tolist()) <= {0.0, 1.0}
            assert torch.equal(torch.isnan(p).any(-1), m == 0) and torch.equal(torch.isnan(p).all(-1), m == 0), name
    p, q, mask = SH.functions_input()
    assert p.shape == q.shape == (4, 2500, 2) and torch.equal(torch.isnan(q).any(-1), mask == 0)


def test_chunks_masks_hold_the_listed_patterns():
    C, W = SH.CHUNK, SH.WAVE
    x, mx, y, my = SH.frames('chunks')
    assert mx.shape == (4, 2500) and my.shape == (4, 1500)
    assert mx.sum(-1).tolist() == [300] * 4 and my.sum(-1).tolist() == [200] * 4
    assert not torch.equal(mx[:, :1500], my)
    # present slots either side of each chunk boundary and at the end
    assert mx[0, [C - 1, C, 2 * C - 1, 2 * C, 2499]].tolist() == [1] * 5 and my[0, [C - 1, C, 1499]].tolist() == [1] * 3
    # a whole chunk with nothing present, later chunks populated
    assert mx[1, C:2 * C].sum() == 0 and mx[1, :C].sum() > 0 and mx[1, 2 * C:].sum() > 0
    assert my[1, :C].sum() == 0 and my[1, C:].sum() == 200
    # a whole wave present next to one wholly absent
    assert mx[2, W:2 * W].all() and mx[2, 2 * W:3 * W].sum() == 0
    assert mx[2, C + 3 * W:C + 4 * W].all() and mx[2, C + 4 * W:C + 5 * W].sum() == 0
    assert my[2, C:C + W].all() and my[2, C + W:C + 2 * W].sum() == 0
    # chunk 0 empty: the first present point lies in chunk 1
    assert mx[3, :C].sum() == 0 and C <= int(mx[3].nonzero()[0]) < 2 * C and mx[3, 2499] == 1
    # holes within every populated chunk, so `before` is never the slot number there
    for m in (mx, my):
        for f in range(4):
            for c0 in range(0, m.shape[1], C):
                k = int(m[f, c0:c0 + C].sum())
                assert k == 0 or k < m[f, c0:c0 + C].numel(), (f, c0)


def test_sparse_counts_and_spread_over_both_chunks():
    C = SH.CHUNK
    x, mx, y, my = SH.frames('sparse')
    assert [(int(a), int(b)) for a, b in zip(mx.sum(-1), my.sum(-1))] == list(SH.SPARSE_COUNTS)
    for f, counts in enumerate(SH.SPARSE_COUNTS):
        for m, c in zip((mx, my), counts):
            if c > 1:
                assert m[f, :C].sum() > 0 and m[f, C:].sum() > 0, (f, c)
    assert int(mx[2].nonzero()[0]) >= C and int(my[3].nonzero()[0]) < C          # the lone points: chunk 1 and chunk 0
    x, mx, y, my, keep = SH.degenerate()
    assert [(int(a), int(b)) for a, b in zip(mx.sum(-1), my.sum(-1))] == \
        [(3, 5), (0, 5), (2, 700), (2, 0), (1, 500), (0, 0), (500, 1), (1, 1)]
    assert torch.equal(mx[keep], SH.frames('sparse')[1])


def test_perm_is_a_scattered_lattice_with_holes():
    x, mx, y, my = SH.frames('perm')
    x2, mx2, y2, my2 = SH.frames('perm_relabelled')
    assert mx.sum() == my.sum() == mx2.sum() == 39 * 39 and not torch.equal(mx, mx2)
    assert torch.equal(y.nan_to_num(-1.0), y2.nan_to_num(-1.0)) and torch.equal(my, my2)
    a, b = SH.compacted('perm', 0)
    a2, _ = SH.compacted('perm_relabelled', 0)
    # the compacted orders differ from the lattice's, from each other and between the sides; the point sets agree
    key = lambda p: sorted(map(tuple, p.tolist()))                                 # noqa: E731
    assert key(a) == key(a2) and not torch.equal(a, a2)
    d = torch.tensor(SH.PERM_D)
    assert key(a + d) == key(b) and not torch.equal(a + d, b)
    # nearest other lattice point is 5 away: every non-matching pair costs at least (5 - 0.3)^2 + 0.2^2 > 22
    C = ((a.double().unsqueeze(1) - b.double().unsqueeze(0)) ** 2).sum(-1)
    second = C.sort(dim=1).values[:, 1].min()
    assert float(second) > 22 and np.allclose(C.min(dim=1).values.numpy(), 0.13, rtol=1e-4)


@pytest.mark.parametrize('name,eps,thresh', SH.GROUPS)
def test_no_frame_stops_within_the_band(name, eps, thresh):
    """At most 2 % of a group's frames may stop within 1e-4 of the threshold: with 3 or 4 frames a group, none."""
    band = SH.band_frames(name, eps, thresh)
    F = SH.n_frames(name)
    print(f'\n{name} eps {eps} thresh {thresh}: {len(band)} of {F} frames in the band; float64 iterations '
          f'{[r[1] for r in SH.ref64(name, eps, thresh)]}')
    assert BAND == 1e-4 and THRESH == SH.REF_THRESH
    assert len(band) <= 0.02 * F
    # the float32 restatement stops where float64 does
    assert [r[1] for r in SH.ref32(name, eps, thresh)] == [r[1] for r in SH.ref64(name, eps, thresh)]


def test_thresh_and_eps_decide_in_these_groups():
    """A kernel that ignored thresh, or eps, would be seen: the float64 iteration counts differ between the groups."""
    its = {(n, e, t): [r[1] for r in SH.ref64(n, e, t)] for n, e, t in SH.GROUPS}
    assert its['sparse', 0.1, 0.1] != its['sparse', 0.1, 1e-3]
    assert its['sparse', 0.1, 0.1] != its['sparse', 1.0, 0.1] and its['small', 0.01, 0.1] != its['small', 0.1, 0.1]
    assert any(1 < i < 100 for v in its.values() for i in v)


def test_functions_input_stays_out_of_the_band():
    from test_metrics_hip_gpu import in_band
    p, q, mask = SH.functions_input()
    for eps in (0.01, 1.0):
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            assert not in_band(sinkhorn64(p[f][sel], q[f][sel], eps=eps)[2]), (eps, f)
    x, y = SH.compacted('chunks', 0)
    assert not in_band(sinkhorn64(x, y, eps=0.01)[2])


def test_sinkhorn32_is_the_package_restatement():
    from piml_amd.functions.metrics import _sinkhorn_torch
    for name, eps in (('small', 0.1), ('small', 0.01), ('sparse', 0.1), ('chunks', 1.0)):
        for f in range(SH.n_frames(name)):
            x, y = SH.compacted(name, f)
            want = float(_sinkhorn_torch(x, y, eps, 100)[0])
            assert SH.ref32(name, eps)[f][0] == want, (name, eps, f)


def test_recorded_values_agree_with_the_float64_restatement():
    """ot64 is the reference on float64 inputs with its float32 log(mu + 1e-8): within 1e-6 of the restatement.  ot32 lies
    within the group's tolerance of it, which is what the GPU test allows the kernel.  MMD: the float64 run within 1e-9
    relative, the float32 run within the existing 1.3e-4."""
    g = golden('metrics_edges')
    for name in ('chunks', 'sparse', 'small'):
        counts = [[a.shape[0], b.shape[0]] for a, b in (SH.compacted(name, f) for f in range(SH.n_frames(name)))]
        assert g[f'{name}/count'].tolist() == counts, name                       # the fixture is of these seeds
        for eps in SH.EPS:
            tol = SH.cost_tolerance(g, name, eps)
            r32, r64 = g[f'{name}/ot32_{eps}'], g[f'{name}/ot64_{eps}']
            print(f'\n{name} eps {eps}: tolerance {tol:.2e}')
            for f, ref in enumerate(SH.ref64(name, eps)):
                if np.isnan(r32[f]):
                    assert counts[f][1] == 1 and np.isnan(r64[f])                  # the reference cannot run one y point
                    continue
                assert abs(r64[f] - ref[0]) <= 1e-6 * abs(ref[0]), (name, eps, f, r64[f], ref[0])
                assert abs(r32[f] - ref[0]) <= tol * abs(ref[0]), (name, eps, f, r32[f], ref[0])
        for f in range(SH.n_frames(name)):
            want = mmd64(*SH.compacted(name, f))
            assert abs(g[f'{name}/mmd64'][f] - want) <= 1e-9 * abs(want), (name, f)
            assert abs(g[f'{name}/mmd32'][f] - want) <= 1.3e-4 * abs(want), (name, f)
    assert np.isnan(g['sparse/ot32_0.1']).sum() == 1


def test_closed_forms_hold_for_the_float64_restatement():
    want = SH.perm_cost()
    assert abs(want - 0.13 * (1 + 1521e-8)) <= 1e-7 * want                        # |d|^2 of the float32 d
    for name in ('perm', 'perm_relabelled'):
        for eps in (0.1, 0.01):
            cost, it, errs = sinkhorn64(*SH.compacted(name, 0), eps=eps)
            assert it == 2 and errs[1] < 1e-9 and abs(cost - want) <= 1e-5 * want, (name, eps, cost, want, errs)
    for f, eps in ((2, 0.1), (2, 1.0), (3, 0.1), (3, 1.0)):
        x, y = SH.compacted('sparse', f)
        assert 1 in (x.shape[0], y.shape[0])
        cost, it, _ = sinkhorn64(x, y, eps=eps)
        want = SH.one_against_many(x, y)
        assert abs(cost - want) <= 1e-9 * want, (f, eps, cost, want)
    # one point a side: the squared distance (its mass 1 + 1e-8 in float64), after 2 iterations
    x, mx, y, my, _ = SH.degenerate()
    a, b = x[7][mx[7] == 1], y[7][my[7] == 1]
    cost, it, _ = sinkhorn64(a, b)
    assert it == 2 and abs(cost - (1 + 1e-8) * float(((a.double() - b.double()) ** 2).sum())) <= 1e-12 * cost


def test_potential_tolerances_are_small():
    """The bound of the GPU test on u, v (3 x the float32 restatement's deviation from float64), printed; v deviates no more
    than the bound made from u allows, so one number serves both."""
    for name in ('chunks', 'small'):
        tol, dv = SH.potential_tolerance(name)
        print(f'\n{name}: potentials within {tol:.2e} (restatement |u32 - u64| {tol / 3:.2e}, |v32 - v64| {dv:.2e})')
        assert 0 < tol < 1e-3 and dv <= tol
