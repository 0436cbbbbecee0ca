"""CPU-only: the Sinkhorn OT / MMD entries of the C ABI (include/piml_hip.h: piml_sinkhorn_frames, piml_mmd_frames) are
declared, exported and bound, reject bad arguments before any HIP call; the operators refuse CPU tensors; and the CPU
forms of the reference's wasserstein_distance_2d / mmd_loss (src/functions/metrics.py:94-104) match its per-frame values
in tests/golden/metrics_frames.npz."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_abi import declared_symbols

SYMS = ('piml_sinkhorn_frames', 'piml_mmd_frames')


def test_entries_declared_exported_and_bound():
    from piml_amd import _lib, build
    build.build()
    L = _lib.lib()
    for name in SYMS:
        assert name in declared_symbols(('piml_hip.h',))
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)


def _sink(L, F=1, n=4, m=4, eps=0.1, max_iter=100, x=1, y=1, cost=1, iters=1):
    return L.piml_sinkhorn_frames(x, y, None, None, F, n, m, eps, max_iter, 0.1, cost, iters, None, None, None)


def _mmd(L, F=1, n=4, m=4, kernel_num=5, x=1, y=1, out=1):
    return L.piml_mmd_frames(x, y, None, None, F, n, m, 2.0, kernel_num, 0.0, out, None)


def test_argument_validation_without_gpu():
    # the fake pointers (1) are never dereferenced: every call below is rejected, or is a no-op, before any HIP call
    from piml_amd import _lib
    L = _lib.lib()
    for bad in (dict(F=-1), dict(n=-1), dict(m=-1), dict(n=4097), dict(m=4097), dict(eps=0.0), dict(eps=-0.1),
                dict(eps=float('nan')), dict(max_iter=-1), dict(x=None), dict(y=None), dict(cost=None), dict(iters=None)):
        assert _sink(L, **bad) == 1, bad
    for bad in (dict(F=-1), dict(n=-1), dict(m=-1), dict(n=4097), dict(m=4097), dict(kernel_num=0), dict(kernel_num=9),
                dict(x=None), dict(y=None), dict(out=None)):
        assert _mmd(L, **bad) == 1, bad
    assert _sink(L, F=0, x=None, y=None, cost=None, iters=None) == 0
    assert _mmd(L, F=0, x=None, y=None, out=None) == 0


def test_ops_and_hip_impl_refuse_cpu_tensors():
    from piml_amd import _lib, ops_metrics
    from piml_amd.functions import metrics as M
    x = torch.zeros(3, 5, 2)
    mask = torch.ones(3, 5)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.sinkhorn_frames(x, x)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.mmd_frames(x, x)
    with pytest.raises(_lib.PimlHipError):
        M.ot_with_time_mask(x, x, mask, reduction='sum', impl='hip')
    with pytest.raises(_lib.PimlHipError):
        M.mmd_with_time_mask(x, x, mask, reduction='sum', impl='hip')
    with pytest.raises(ValueError):
        M.ot_with_time_mask(x, x, mask, reduction='sum', impl='cuda')


def test_cpu_wasserstein_and_mmd_loss_match_reference_frames():
    """OT within 1e-6 relative (float32, the reference's own arithmetic); MMD, evaluated in float64, within 3x the
    reference's own float32-vs-float64 spread on that frame (absolute floor 1e-8)."""
    from piml_amd.functions import metrics as M
    g = golden('metrics_frames')
    for name in ('gc', 'ucy', 'syn512', 'edge'):
        p, q, mask = g[f'{name}/p'], g[f'{name}/q'], g[f'{name}/mask']
        for f in range(p.shape[0]):
            sel = mask[f] == 1
            if sel.sum() < 2:
                continue
            x, y = torch.tensor(p[f][sel]), torch.tensor(q[f][sel])
            ot, mmd32, mmd64 = g[f'{name}/ot'][f], g[f'{name}/mmd32'][f], g[f'{name}/mmd64'][f]
            dist, _, _ = M.wasserstein_distance_2d(x, y)
            assert abs(float(dist) - ot) <= 1e-6 * abs(ot), (name, f, float(dist), ot)
            got = float(M.mmd_loss(x, y))
            if np.isnan(mmd32):
                assert np.isnan(got), (name, f)
                continue
            assert abs(got - mmd32) <= max(3 * abs(mmd32 - mmd64), 1e-8), (name, f, got, mmd32, mmd64)


def test_cpu_wasserstein_unequal_sizes_and_batched_input():
    from piml_amd.functions import metrics as M
    g = golden('metrics_frames')
    for k in range(2):
        x, y = torch.tensor(g[f'uneq{k}/x']), torch.tensor(g[f'uneq{k}/y'])
        dist, P, C = M.wasserstein_distance_2d(x, y)
        assert P.shape == (x.shape[0], y.shape[0]) and C.shape == P.shape
        assert abs(float(dist) - float(g[f'uneq{k}/dist'])) <= 1e-6 * abs(float(g[f'uneq{k}/dist']))
        assert np.allclose(C.numpy(), g[f'uneq{k}/C'], rtol=1e-6, atol=0)
        assert np.allclose(P.numpy(), g[f'uneq{k}/P'], rtol=1e-5, atol=1e-12)
        mmd32, mmd64 = float(g[f'uneq{k}/mmd32']), float(g[f'uneq{k}/mmd64'])
        assert abs(float(M.mmd_loss(x, y)) - mmd32) <= max(3 * abs(mmd32 - mmd64), 1e-8)
    # 3-D (batched) input takes the torch restatement, which stops the batch on the MEAN err of its frames as the
    # reference does (metrics.py:168), not per frame
    x, y = torch.tensor(g['batch/x']), torch.tensor(g['batch/y'])
    dist, P, C = M.wasserstein_distance_2d(x, y)
    assert dist.shape == (3,) and P.shape == (3, 30, 40) and C.shape == (3, 30, 40)
    assert np.allclose(dist.numpy(), g['batch/dist'], rtol=1e-6, atol=0)
    per_frame = np.array([float(M.wasserstein_distance_2d(x[b], y[b])[0]) for b in range(3)])
    assert not np.allclose(per_frame, g['batch/dist'], rtol=1e-6, atol=0)      # the coupling is visible in this batch


def test_stats_wrappers_refuse_inputs_on_another_device():
    """every *_stats_frames wrapper (and both group passes) raises ValueError, before any library call, when V, M, the
    obstacle points, the lines or n_active are not on P's device: tensors of two fake devices, so no GPU is needed"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from piml_amd import ops_metrics as OM
    S, T, N = 2, 3, 4
    with FakeTensorMode():
        def f32(dev, *shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)
        P, V, M = f32('cuda:0', S, T, N, 2), f32('cuda:0', S, T, N, 2), f32('cuda:0', S, T, N)
        V1, M1 = f32('cuda:1', S, T, N, 2), f32('cuda:1', S, T, N)
        obs, obs1, lines, lines1 = f32('cuda:0', 5, 2), f32('cuda:1', 5, 2), f32('cuda:0', 2, 4), f32('cuda:1', 2, 4)
        n1 = torch.empty(S, device='cuda:1', dtype=torch.int32)
        box = dict(box=(0.0, 1.0, 0.0, 1.0), grid=(2, 2))
        for fn, kw in ((OM.crowd_stats_frames, {}), (OM.crowd_stats_voronoi_frames, dict(dirs=np.zeros((4, 2), np.float32))),
                       (OM.pair_stats_frames, {}), (OM.flow_stats_frames, box), (OM.view_stats_frames, {})):
            for args in ((P, V1, M), (P, V, M1)):
                with pytest.raises(ValueError, match='P, V and M on different devices'):
                    fn(*args, **kw)
            with pytest.raises(ValueError, match='n_active: expected an int32'):
                fn(P, V, M, n_active=n1, **kw)
        for args in ((P, V1, M, obs), (P, V, M1, obs), (P, V, M, obs1)):
            with pytest.raises(ValueError, match='P, V, M and obstacles on different devices'):
                OM.obstacle_stats_frames(*args)
        for args in ((P, M1, lines), (P, M, lines1)):
            with pytest.raises(ValueError, match='P, M and lines on different devices'):
                OM.line_stats_frames(*args)
        for fn, args in ((OM.track_stats_frames, ()), (OM.group_pairs_frames, (1.0, 1.0, 1.0, 1)),
                         (OM.group_members_frames, (torch.empty(0, 3, device='cuda:0', dtype=torch.int32), 1.0, 1.0, 1.0))):
            with pytest.raises(ValueError, match='P and M on different devices'):
                fn(P, M1, *args)
        for fn, args in ((OM.obstacle_stats_frames, (P, V, M, obs)), (OM.line_stats_frames, (P, M, lines)),
                         (OM.track_stats_frames, (P, M)), (OM.group_pairs_frames, (P, M, 1.0, 1.0, 1.0, 1))):
            with pytest.raises(ValueError, match='n_active: expected an int32'):
                fn(*args, n_active=n1)
