"""GPU: the Sinkhorn OT and MMD kernels (piml_amd/csrc/metrics.hip) per frame against the reference's per-frame values
(tests/golden/metrics_frames.npz) and against float64 restatements written here, the edge cases of the C ABI's contract,
determinism and graph capture, the reference's wasserstein_distance_2d / mmd_loss on GPU tensors, and the evaluation of
BaseSimulator.test_multiple_rollouts with metrics_impl='hip' against 'torch'."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SETS = ('gc', 'ucy', 'syn512', 'syn1024', 'edge')
THRESH = 0.1
BAND = 1e-4


def sinkhorn64(x, y, eps=0.1, max_iter=100, thresh=THRESH, potentials=False):
    """SinkhornDistance.forward (src/functions/metrics.py:129-187) on one frame in float64: (cost, iterations, [err of
    every iteration run]) and, with potentials, the final u and v"""
    x, y = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64)
    C = ((x.unsqueeze(-2) - y.unsqueeze(-3)) ** 2).sum(-1)
    lmu, lnu = np.log(1.0 / x.shape[0] + 1e-8), np.log(1.0 / y.shape[0] + 1e-8)
    u, v = torch.zeros_like(x[:, 0]), torch.zeros_like(y[:, 0])
    errs = []
    for _ in range(max_iter):
        un = eps * (lmu - torch.logsumexp((-C + u.unsqueeze(-1) + v.unsqueeze(-2)) / eps, dim=-1)) + u
        v = eps * (lnu - torch.logsumexp((-C + un.unsqueeze(-1) + v.unsqueeze(-2)) / eps, dim=-2)) + v
        errs.append(float((un - u).abs().sum()))
        u = un
        if errs[-1] < thresh:
            break
    out = float((torch.exp((-C + u.unsqueeze(-1) + v.unsqueeze(-2)) / eps) * C).sum()), len(errs), errs
    return out + (u, v) if potentials else out


def mmd64(x, y, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """MaximumMeanDiscrepancy (src/functions/metrics.py:207-273) on one frame in float64"""
    from piml_amd.functions.metrics import _mmd_torch
    return float(_mmd_torch(torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64),
                            kernel_mul, kernel_num, fix_sigma))


def in_band(errs, thresh=THRESH):
    """float64's err at the stopping iteration (or the one before it) within BAND of the threshold: float32 may stop
    one iteration apart"""
    return any(abs(e - thresh) < BAND for e in errs[-2:])


def frames(g, name):
    p, q, mask = g[f'{name}/p'], g[f'{name}/q'], g[f'{name}/mask']
    return p, q, mask


def gpu(*arrs):
    return [torch.tensor(a, device=DEV) for a in arrs]


def test_ot_per_frame_and_iteration_counts():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    rows, band = [], 0
    for name in SETS:
        p, q, mask = frames(g, name)
        cost, iters = ops_metrics.sinkhorn_frames(*gpu(p, q, mask, mask))
        cost, iters = cost.cpu().numpy().astype(np.float64), iters.cpu().numpy()
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            if sel.sum() < 2:
                continue
            want64, it64, errs = sinkhorn64(p[f][sel], q[f][sel])
            ref = g[f'{name}/ot'][f]
            rel = abs(cost[f] - ref) / max(abs(ref), 1e-30)
            if in_band(errs):
                band += 1
                assert abs(int(iters[f]) - it64) <= 1, (name, f, iters[f], it64)
            else:
                assert iters[f] == it64, (name, f, iters[f], it64, errs[-2:])
                assert abs(cost[f] - ref) <= 1e-5 * abs(ref), (name, f, cost[f], ref)
            rows.append((name, f, int(sel.sum()), int(iters[f]), rel, abs(want64 - ref) / max(abs(ref), 1e-30)))
    print(f'\n{len(rows)} frames, {band} within {BAND} of the threshold; worst rel vs reference '
          f'{max(r[4] for r in rows):.2e} (reference float32 vs float64: {max(r[5] for r in rows):.2e})')
    assert band <= 0.02 * len(rows)


def test_mmd_per_frame_against_float64_and_reference():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    worst64 = worst_ref = 0.0
    for name in SETS:
        p, q, mask = frames(g, name)
        out = ops_metrics.mmd_frames(*gpu(p, q, mask, mask)).cpu().numpy().astype(np.float64)
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            if sel.sum() < 2:
                continue
            want = mmd64(p[f][sel], q[f][sel])
            r32, r64 = g[f'{name}/mmd32'][f], g[f'{name}/mmd64'][f]
            if np.isnan(want):
                assert np.isnan(out[f]) and np.isnan(r32), (name, f)
                continue
            assert abs(out[f] - want) <= max(1e-5 * abs(want), 1e-9), (name, f, out[f], want)
            assert abs(out[f] - r32) <= max(3 * abs(r32 - r64), 1e-8), (name, f, out[f], r32, r64)
            worst64 = max(worst64, abs(out[f] - want) / abs(want))
            worst_ref = max(worst_ref, abs(out[f] - r32) / max(abs(r32 - r64), 1e-30))
    print(f'\nMMD: worst rel vs float64 {worst64:.2e}; worst |hip - ref32| / |ref32 - ref64| {worst_ref:.2f}')


def test_hip_aggregates_on_metrics_fixture():
    from piml_amd.functions import metrics as M
    g = golden('metrics')
    p, q, mask = gpu(g['p'], g['q'], g['mask'])
    for red in ('sum', 'mean'):
        assert np.isclose(M.ot_with_time_mask(p, q, mask, reduction=red, impl='hip'), float(g[f'ot_{red}']), rtol=1e-6, atol=0)
        assert np.isclose(M.mmd_with_time_mask(p, q, mask, reduction=red, impl='hip'), float(g[f'mmd_{red}']),
                          rtol=1.3e-4, atol=0)
    # reduction=None: one value per frame with more than one agent, as impl='torch' gives
    assert len(M.ot_with_time_mask(p, q, mask, impl='hip')) == len(M.ot_with_time_mask(p, q, mask))
    assert len(M.mmd_with_time_mask(p, q, mask, impl='hip')) == len(M.mmd_with_time_mask(p, q, mask))


def test_absent_slots_holding_nan_and_nan_in_present_points():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    p, q, mask = frames(g, 'gc')
    assert np.isnan(p[mask == 0]).all()                                  # the fixture's absent slots hold NaN
    clean_p, clean_q = np.where(mask[..., None] == 1, p, 123.0), np.where(mask[..., None] == 1, q, -7.0)
    a = ops_metrics.sinkhorn_frames(*gpu(p, q, mask, mask))
    b = ops_metrics.sinkhorn_frames(*gpu(clean_p, clean_q, mask, mask))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops_metrics.mmd_frames(*gpu(p, q, mask, mask)), ops_metrics.mmd_frames(*gpu(clean_p, clean_q, mask, mask)))
    # a NaN in a PRESENT point: that frame's OT and MMD are NaN, its Sinkhorn runs all max_iter iterations
    bad = p.copy()
    k = int(np.nonzero(mask[3])[0][5])
    bad[3, k, 0] = np.nan
    cost, iters = ops_metrics.sinkhorn_frames(*gpu(bad, q, mask, mask), max_iter=37)
    mmd = ops_metrics.mmd_frames(*gpu(bad, q, mask, mask))
    assert torch.isnan(cost[3]) and int(iters[3]) == 37 and torch.isnan(mmd[3])
    others = [f for f in range(p.shape[0]) if f != 3]
    assert not torch.isnan(cost[others]).any() and not torch.isnan(mmd[others]).any()


def test_identical_points_fix_sigma_and_kernel_num():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    p, q, mask = frames(g, 'edge')
    out = ops_metrics.mmd_frames(*gpu(p, q, mask, mask)).cpu().numpy()
    assert np.isnan(out[3]) and np.isnan(g['edge/mmd32'][3])            # all points coincide: bandwidth 0 -> NaN
    p, q, mask = frames(g, 'gc')
    for kw in (dict(fix_sigma=2.5), dict(fix_sigma=0), dict(kernel_num=1), dict(kernel_num=3), dict(kernel_num=8),
               dict(kernel_mul=3.0, kernel_num=4, fix_sigma=0.7)):
        out = ops_metrics.mmd_frames(*gpu(p, q, mask, mask), **kw).cpu().numpy().astype(np.float64)
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            want = mmd64(p[f][sel], q[f][sel], **kw)
            assert abs(out[f] - want) <= max(1e-5 * abs(want), 1e-9), (kw, f, out[f], want)
    # fix_sigma = 0 is Python-falsy: the bandwidth of the data, the same bits as None
    a = ops_metrics.mmd_frames(*gpu(p, q, mask, mask), fix_sigma=0)
    assert torch.equal(a, ops_metrics.mmd_frames(*gpu(p, q, mask, mask)))


def test_max_iter_one_and_zero():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    p, q, mask = frames(g, 'ucy')
    for max_iter in (1, 0):
        cost, iters = ops_metrics.sinkhorn_frames(*gpu(p, q, mask, mask), max_iter=max_iter)
        assert (iters == max_iter).all()
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            want, it, _ = sinkhorn64(p[f][sel], q[f][sel], max_iter=max_iter)
            assert it == max_iter and abs(float(cost[f]) - want) <= 1e-5 * abs(want), (max_iter, f, float(cost[f]), want)


def test_leading_dims_and_non_contiguous_views():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    p, q, mask = gpu(*frames(g, 'gc'))
    cost, iters, u, v = ops_metrics.sinkhorn_frames(p, q, mask, mask, want_potentials=True)
    mmd = ops_metrics.mmd_frames(p, q, mask, mask)
    # (*c) = (3, 4)
    c4 = ops_metrics.sinkhorn_frames(p.reshape(3, 4, -1, 2), q.reshape(3, 4, -1, 2), mask.reshape(3, 4, -1),
                                     mask.reshape(3, 4, -1), want_potentials=True)
    assert c4[0].shape == (3, 4) and c4[2].shape == (3, 4, p.shape[1])
    for a, b in zip(c4, (cost, iters, u, v)):
        assert torch.equal(a.reshape(b.shape), b)
    assert torch.equal(ops_metrics.mmd_frames(p.reshape(3, 4, -1, 2), q.reshape(3, 4, -1, 2), mask.reshape(3, 4, -1),
                                              mask.reshape(3, 4, -1)).reshape(-1), mmd)
    # non-contiguous views: every other frame, and coordinates from a wider (.., 3) tensor
    wide_p = torch.cat((p, torch.zeros_like(p[..., :1])), -1)[..., :2]
    assert not wide_p.is_contiguous()
    assert torch.equal(ops_metrics.sinkhorn_frames(wide_p[::2], q[::2], mask[::2], mask[::2])[0], cost[::2])
    assert torch.equal(ops_metrics.mmd_frames(wide_p[::2], q[::2], mask[::2], mask[::2]), mmd[::2])
    # the potentials are 0 at absent slots
    assert (u[mask == 0] == 0).all() and (v[mask == 0] == 0).all()


def test_largest_frame_accepted_next_rejected():
    from piml_amd import _lib, ops_metrics
    gen = torch.Generator().manual_seed(5)
    x = (20 * torch.rand(1, 4096, 2, generator=gen)).to(DEV)
    y = x + 0.3 * torch.randn(1, 4096, 2, generator=gen).to(DEV)
    cost, iters = ops_metrics.sinkhorn_frames(x, y, max_iter=3)
    want, _, _ = sinkhorn64(x[0], y[0], max_iter=3)                     # float64 on the GPU: 4096 x 4096
    assert int(iters[0]) == 3 and abs(float(cost[0]) - want) <= 1e-5 * abs(want), (float(cost[0]), want)
    mmd = float(ops_metrics.mmd_frames(x, y)[0])
    want = mmd64(x[0], y[0])
    assert abs(mmd - want) <= max(1e-5 * abs(want), 1e-9), (mmd, want)
    big = torch.zeros(1, 4097, 2, device=DEV)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.sinkhorn_frames(big, x)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.mmd_frames(x, big)


def test_empty_selections_return_what_torch_returns():
    from piml_amd.functions import metrics as M
    p = torch.zeros(5, 6, 2, device=DEV)
    for mask in (torch.zeros(5, 6, device=DEV), torch.eye(5, 6, device=DEV)):      # no frame with more than one agent
        for red in ('sum', 'mean', None):
            for fn in (M.ot_with_time_mask, M.mmd_with_time_mask):
                a, b = fn(p, p, mask, reduction=red), fn(p, p, mask, reduction=red, impl='hip')
                assert (np.isnan(a) and np.isnan(b)) if red == 'mean' else a == b, (fn.__name__, red, a, b)


def test_deterministic_and_graph_capture_replays_eager_bits():
    from piml_amd import ops_metrics
    g = golden('metrics_frames')
    p, q, mask = gpu(*frames(g, 'syn512'))
    run = lambda: (ops_metrics.sinkhorn_frames(p, q, mask, mask, want_potentials=True),          # noqa: E731
                   ops_metrics.mmd_frames(p, q, mask, mask))
    (a, am), (b, bm) = run(), run()
    for x, y in zip(a + (am,), b + (bm,)):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c, cm = run()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a + (am,), c + (cm,)):
        assert torch.equal(x, y)


def test_wasserstein_distance_2d_and_mmd_loss_unequal_sizes():
    from piml_amd.functions import metrics as M
    g = golden('metrics_frames')
    for k in range(2):
        x, y = gpu(g[f'uneq{k}/x'], g[f'uneq{k}/y'])
        dist, P, C = M.wasserstein_distance_2d(x, y)
        assert dist.is_cuda and dist.dim() == 0
        want = float(g[f'uneq{k}/dist'])
        assert abs(float(dist) - want) <= 1e-5 * abs(want), (k, float(dist), want)
        Pw, Cw = g[f'uneq{k}/P'], g[f'uneq{k}/C']
        assert np.abs(C.cpu().numpy() - Cw).max() <= 1e-5 * np.abs(Cw).max()
        assert np.abs(P.cpu().numpy() - Pw).max() <= 1e-5 * np.abs(Pw).max()
        r32, r64 = float(g[f'uneq{k}/mmd32']), float(g[f'uneq{k}/mmd64'])
        got = float(M.mmd_loss(x, y))
        assert abs(got - r32) <= max(3 * abs(r32 - r64), 1e-8), (k, got, r32, r64)
    # 3-D input on the GPU: the torch restatement with the reference's batch-mean stop
    x, y = gpu(g['batch/x'], g['batch/y'])
    assert np.allclose(M.wasserstein_distance_2d(x, y)[0].cpu().numpy(), g['batch/dist'], rtol=1e-5, atol=0)


def test_multiple_rollouts_evaluation_hip_against_torch():
    from test_simulator_gpu import load_data, make_sim, sim_args
    g = golden('rollout')
    res = {}
    for impl in ('torch', 'hip'):
        sim = make_sim(g, sim_args(metrics_impl=impl), 'sd_m/')
        out = sim.test_multiple_rollouts([load_data(g, 'roll')], load_model=False)
        res[impl] = (out, dict(sim.last_eval))
    (t, te), (h, he) = res['torch'], res['hip']
    for k in ('loss', 'mse', 'mae', 'fde', 'collisions', 'hard_collisions'):
        assert te[k] == he[k], (k, te[k], he[k])
    assert abs(he['ot'] - te['ot']) <= 1e-5 * abs(te['ot']), (he['ot'], te['ot'])
    assert abs(he['mmd'] - te['mmd']) <= 1.3e-4 * abs(te['mmd']), (he['mmd'], te['mmd'])
    print(f"\nevaluation ot torch {te['ot']!r} hip {he['ot']!r}; mmd torch {te['mmd']!r} hip {he['mmd']!r}")
