"""Evaluation metrics on the hot path's side (src/functions/metrics.py:16-104): collision counts via
the fused HIP kernel, the masked mean displacement error (MAE = ADE-equivalent), and Sinkhorn OT / MMD either as
batched torch (impl='torch', the default) or on the per-frame HIP kernels of ops_metrics (impl='hip')."""
import torch

from .. import ops


def collision_count(position, threshold, real_position=None, reduction=None):
    """Pedestrians.collision_detection reduced over everything (metrics.py:16-26).  'sum' / 'mean'
    use the fused per-agent count kernel (no (t,n,n) matrix) when no `real_position` is given;
    reduction=None returns the matrix like the reference."""
    if reduction is None:
        return ops.collision_detection(position, threshold, real_position)
    if reduction not in ('sum', 'mean'):
        raise NotImplementedError
    if real_position is not None or position.dim() != 3:
        total = ops.collision_detection(position, threshold, real_position).sum()
    else:
        total = ops.collision_counts(position, (threshold,))[0].sum()
    n = position.shape[-2]
    cells = position.numel() // 2 * n
    return (total if reduction == 'sum' else total / cells).item()


def mae_with_time_mask(p_pred, labels, mask_p_pred, reduction='none'):
    """Mean L2 displacement over the masked (frame, agent) entries (metrics.py:29-42)."""
    m = mask_p_pred == 1
    err = torch.norm(torch.where(m.unsqueeze(-1), p_pred - labels, torch.zeros_like(p_pred)), p=2, dim=-1)
    if reduction == 'sum':
        return err.sum().item()
    if reduction == 'mean':
        return (err.sum() / m.sum().clamp(min=1)).item()
    return err


def _per_frame(p, q, mask):
    """(*c, t, n, d), mask (*c, t, n) -> frames flattened: (F, n, d), (F, n, d), bool (F, n)."""
    n = mask.shape[-1]
    return p.reshape(-1, n, p.shape[-1]), q.reshape(-1, n, q.shape[-1]), (mask == 1).reshape(-1, n)


def _reduce(vals, reduction):
    """per-frame float32 values -> the reference's np.sum / np.mean of the list (float64), or the list"""
    if reduction == 'sum':
        return vals.double().sum().item()
    if reduction == 'mean':
        return vals.double().mean().item()
    return vals.tolist()


def _check_impl(impl):
    if impl not in ('torch', 'hip'):
        raise ValueError(f"impl must be 'torch' or 'hip', got {impl!r}")
    return impl == 'hip'


def _selected_frames(p, q, mask):
    """the frames with more than one present agent: (F, n, 2), (F, n, 2), bool (F, n)"""
    x, y, m = _per_frame(p.detach(), q.detach(), mask)
    use = m.sum(-1) > 1
    return x[use], y[use], m[use]


def ot_with_time_mask(p, q, mask, eps=0.1, max_iter=100, reduction=None, dvs=None, impl='torch'):
    """Entropic OT (log-domain Sinkhorn) between the predicted and the true positions of the agents
    present in each frame (metrics.py:45-67, 107-203), all frames batched: absent agents are masked
    out of the marginals and every frame stops updating at its own iteration, exactly where the
    reference's per-frame loop breaks (err < 0.1).  Frames with fewer than 2 agents are skipped.
    impl='hip': every selected frame in one launch of the Sinkhorn kernel (ops_metrics.sinkhorn_frames)."""
    if _check_impl(impl):
        from .. import ops_metrics
        x, y, m = _selected_frames(p, q, mask)
        if x.shape[0] == 0:
            return 0.0 if reduction == 'sum' else (float('nan') if reduction == 'mean' else [])
        return _reduce(ops_metrics.sinkhorn_frames(x, y, m, m, eps=eps, max_iter=max_iter)[0], reduction)
    x, y, m = _per_frame(p.detach(), q.detach(), mask)
    cnt = m.sum(-1)
    use = cnt > 1
    x, y, m, cnt = x[use], y[use], m[use], cnt[use]
    if x.shape[0] == 0:
        return 0.0 if reduction in ('sum',) else (float('nan') if reduction == 'mean' else [])
    x = torch.where(m.unsqueeze(-1), x, torch.zeros_like(x))
    y = torch.where(m.unsqueeze(-1), y, torch.zeros_like(y))
    C = ((x.unsqueeze(-2) - y.unsqueeze(-3)).abs() ** 2).sum(-1)                    # F, n, n
    pair = m.unsqueeze(-1) & m.unsqueeze(-2)
    neg = torch.full_like(C, float('-inf'))
    logw = torch.log(1.0 / cnt.to(C.dtype) + 1e-8).unsqueeze(-1)                    # log(mu + 1e-8)
    u = torch.zeros_like(x[..., 0])
    v = torch.zeros_like(u)

    def M(u_, v_):
        return torch.where(pair, (-C + u_.unsqueeze(-1) + v_.unsqueeze(-2)) / eps, neg)
    active = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
    for _ in range(max_iter):
        u_new = eps * (logw - torch.logsumexp(M(u, v), dim=-1)) + u
        u_new = torch.where(m, u_new, torch.zeros_like(u_new))
        v_new = eps * (logw - torch.logsumexp(M(u_new, v).transpose(-2, -1), dim=-1)) + v
        v_new = torch.where(m, v_new, torch.zeros_like(v_new))
        err = (u_new - u).abs().sum(-1)
        a = active.unsqueeze(-1)
        u, v = torch.where(a, u_new, u), torch.where(a, v_new, v)
        active = active & ~(err < 1e-1)
        if not bool(active.any()):
            break
    pi = torch.where(pair, torch.exp(M(u, v)), torch.zeros_like(C))
    cost = (pi * C).sum(dim=(-2, -1))
    if reduction == 'sum':
        return cost.sum().item()
    if reduction == 'mean':
        return cost.mean().item()
    return cost.tolist()


def mmd_with_time_mask(p, q, mask, kernel_mul=2.0, kernel_num=5, fix_sigma=None, reduction=None, impl='torch'):
    """Multi-kernel Gaussian MMD between predicted and true positions per frame
    (metrics.py:70-91, 207-273), all frames batched with masks.  impl='hip': every selected frame in one
    launch of the MMD kernel (ops_metrics.mmd_frames, float64 inside)."""
    if _check_impl(impl):
        from .. import ops_metrics
        x, y, m = _selected_frames(p, q, mask)
        if x.shape[0] == 0:
            return 0.0 if reduction == 'sum' else (float('nan') if reduction == 'mean' else [])
        return _reduce(ops_metrics.mmd_frames(x, y, m, m, kernel_mul, kernel_num, fix_sigma), reduction)
    x, y, m = _per_frame(p.detach(), q.detach(), mask)
    cnt = m.sum(-1)
    use = cnt > 1
    x, y, m, cnt = x[use], y[use], m[use], cnt[use].to(x.dtype)
    if x.shape[0] == 0:
        return 0.0 if reduction == 'sum' else (float('nan') if reduction == 'mean' else [])
    total = torch.cat((torch.where(m.unsqueeze(-1), x, torch.zeros_like(x)),
                       torch.where(m.unsqueeze(-1), y, torch.zeros_like(y))), dim=1)          # F, 2n, d
    mm = torch.cat((m, m), dim=1)
    pair = (mm.unsqueeze(-1) & mm.unsqueeze(-2)).to(x.dtype)
    L2 = ((total.unsqueeze(1) - total.unsqueeze(2)) ** 2).sum(-1) * pair
    ns = 2 * cnt
    bandwidth = fix_sigma if fix_sigma else L2.sum(dim=(-2, -1)) / (ns ** 2 - ns)
    bandwidth = bandwidth / kernel_mul ** (kernel_num // 2)
    K = sum(torch.exp(-L2 / (bandwidth * kernel_mul ** i).reshape(-1, 1, 1)) for i in range(kernel_num)) * pair
    n = x.shape[1]
    n2 = (cnt * cnt).reshape(-1, 1, 1)
    loss = (K[:, :n, :n] / n2).sum(dim=(-2, -1)) - (K[:, :n, n:] / n2).sum(dim=(-2, -1)) \
        - (K[:, n:, :n] / n2).sum(dim=(-2, -1)) + (K[:, n:, n:] / n2).sum(dim=(-2, -1))
    if reduction == 'sum':
        return loss.sum().item()
    if reduction == 'mean':
        return loss.mean().item()
    return loss.tolist()


def fde_with_time_mask(p_pred, labels, mask_p_pred, reduction='mean'):
    """Final displacement error: L2 error at each agent's LAST masked frame of a (t, n, 2) rollout.
    The reference only reports the mean displacement (its "MAE", = ADE); BASELINE.json's config 5
    asks for ADE/FDE, so the FDE of the same masks is provided alongside."""
    m = mask_p_pred == 1                                                     # t, n
    T = m.shape[0]
    ar = torch.arange(T, device=m.device).unsqueeze(1)
    last = torch.where(m, ar, -1).max(0).values                              # n, -1 = never predicted
    has = last >= 0
    idx = last.clamp(min=0)
    cols = torch.arange(m.shape[1], device=m.device)
    err = torch.norm(p_pred[idx, cols] - labels[idx, cols], p=2, dim=-1)
    err = torch.where(has, torch.nan_to_num(err), torch.zeros_like(err))
    if reduction == 'sum':
        return err.sum().item()
    if reduction == 'mean':
        return (err.sum() / has.sum().clamp(min=1)).item()
    return err


def _cost_matrix(x, y):
    """|x_i - y_j|^2 summed over the coordinates (SinkhornDistance._cost_matrix, metrics.py:184-190)"""
    return ((x.unsqueeze(-2) - y.unsqueeze(-3)).abs() ** 2).sum(-1)


def _sinkhorn_torch(x, y, eps, max_iter):
    """SinkhornDistance.forward (metrics.py:129-187) restated in torch, float32 like the reference: for 3-D (batched)
    input the loop stops on the batch-MEAN err (metrics.py:168), which couples the frames.  -> (cost, pi, C)"""
    C = _cost_matrix(x, y)
    lead = x.shape[:-2]
    log_mu = torch.log(torch.full((*lead, x.shape[-2]), 1.0 / x.shape[-2], dtype=torch.float32, device=x.device) + 1e-8)
    log_nu = torch.log(torch.full((*lead, y.shape[-2]), 1.0 / y.shape[-2], dtype=torch.float32, device=x.device) + 1e-8)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)

    def M(u_, v_):
        return (-C + u_.unsqueeze(-1) + v_.unsqueeze(-2)) / eps
    for _ in range(max_iter):
        u_prev = u
        u = eps * (log_mu - torch.logsumexp(M(u, v), dim=-1)) + u
        v = eps * (log_nu - torch.logsumexp(M(u, v).transpose(-2, -1), dim=-1)) + v
        if (u - u_prev).abs().sum(-1).mean().item() < 0.1:
            break
    pi = torch.exp(M(u, v))
    return (pi * C).sum(dim=(-2, -1)), pi, C


def wasserstein_distance_2d(distribution_p, distribution_q, eps=0.1, max_iter=100, reduction=None):
    """metrics.py:94-97: (dist, P, C) of the entropic OT between two point clouds (n, 2) and (m, 2), n != m allowed.
    On GPU tensors the cost and the potentials come from the Sinkhorn kernel (ops_metrics.sinkhorn_frames) and P is
    formed from them by torch with the reference's expression.  CPU tensors, and 3-D (batched) input on any device, take
    the torch restatement: the reference stops a batch on the MEAN err of its frames, which the per-frame kernel does
    not do."""
    x, y = distribution_p, distribution_q
    if x.is_cuda and x.dim() == 2:
        from .. import ops_metrics
        dist, _, u, v = ops_metrics.sinkhorn_frames(x, y, eps=eps, max_iter=max_iter, want_potentials=True)
        C = _cost_matrix(x, y)
        P = torch.exp((-C + u.unsqueeze(-1) + v.unsqueeze(-2)) / eps)
    else:
        dist, P, C = _sinkhorn_torch(x, y, eps, max_iter)
    if reduction == 'mean':
        dist = dist.mean()
    elif reduction == 'sum':
        dist = dist.sum()
    return dist, P, C


def _mmd_torch(x, y, kernel_mul, kernel_num, fix_sigma):
    """MaximumMeanDiscrepancy.__call__ (metrics.py:207-273) restated in torch on (n, d), (m, d), in float64 like the
    kernel (the float32 evaluation carries ~4e-5 of cancellation error)"""
    n, m = x.shape[0], y.shape[0]
    total = torch.cat((x, y), dim=0).double()
    L2 = ((total.unsqueeze(0) - total.unsqueeze(1)) ** 2).sum(-1)
    bandwidth = fix_sigma if fix_sigma else L2.sum() / ((n + m) ** 2 - (n + m))
    bandwidth = bandwidth / kernel_mul ** (kernel_num // 2)
    K = sum(torch.exp(-L2 / (bandwidth * kernel_mul ** i)) for i in range(kernel_num))
    return (K[:n, :n] / (n * n)).sum() - (K[:n, n:] / (n * m)).sum() - (K[n:, :n] / (m * n)).sum() \
        + (K[n:, n:] / (m * m)).sum()


def mmd_loss(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """metrics.py:100-104: the MMD of two point clouds (n, 2) and (m, 2) as a 0-d tensor of source's dtype.  GPU
    tensors run the MMD kernel (ops_metrics.mmd_frames), CPU tensors the float64 torch restatement."""
    if source.is_cuda:
        from .. import ops_metrics
        return ops_metrics.mmd_frames(source.unsqueeze(0), target.unsqueeze(0), kernel_mul=kernel_mul,
                                      kernel_num=kernel_num, fix_sigma=fix_sigma)[0]
    return _mmd_torch(source, target, kernel_mul, kernel_num, fix_sigma).to(source.dtype)
