"""Evaluation-metric operators over the C ABI (include/piml_hip.h: piml_sinkhorn_frames, piml_mmd_frames).

Entropic OT and multi-kernel MMD of point clouds, every frame in one launch.  Like every operator of piml_amd they
require float32 GPU tensors and raise PimlHipError on CPU ones; functions/metrics.py builds the reference's interface on
them."""
import torch

from . import _lib
from .ops import _gpu_f32, _ptr, _stream


def _frames(name, t):
    """(*c, n, 2) -> contiguous (F, n, 2) and the leading shape (n <= 4096 is the library's check)."""
    t = _gpu_f32(name, t.detach())
    if t.dim() < 2 or t.shape[-1] != 2:
        raise ValueError(f'{name}: expected (*c, n, 2), got {tuple(t.shape)}')
    lead = t.shape[:-2]
    return t.reshape(lead.numel(), t.shape[-2], 2), lead


def _mask(name, mask, x):
    """None, or (*c, n) presence (non-zero = present) -> uint8 (F, n) on x's device."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.device != x.device:
        raise _lib.PimlHipError(f'{name}: expected a tensor on {x.device}, got {getattr(mask, "device", type(mask))}')
    if mask.numel() != x.shape[0] * x.shape[1]:
        raise ValueError(f'{name}: {tuple(mask.shape)} does not match {x.shape[0]} frames of {x.shape[1]} points')
    return (mask != 0).to(torch.uint8).reshape(x.shape[0], x.shape[1])


def _pair(x, y, mask_x, mask_y):
    x, lead = _frames('x', x)
    y, lead_y = _frames('y', y)
    if lead != lead_y:
        raise ValueError(f'x and y frames differ: {tuple(lead)} vs {tuple(lead_y)}')
    if x.device != y.device:
        raise ValueError('x and y on different devices')
    return x, y, _mask('mask_x', mask_x, x), _mask('mask_y', mask_y, y), lead


def sinkhorn_frames(x, y, mask_x=None, mask_y=None, eps=0.1, max_iter=100, thresh=0.1, want_potentials=False):
    """Entropic OT cost of every frame (SinkhornDistance, src/functions/metrics.py:107-187, per frame): x (*c, n, 2),
    y (*c, m, 2), optional presence masks (*c, n) / (*c, m).  Returns (cost (*c) float32, iters (*c) int32) and, with
    want_potentials, the potentials u (*c, n) and v (*c, m) (0 at absent points)."""
    x, y, mx, my, lead = _pair(x, y, mask_x, mask_y)
    F, n, m = x.shape[0], x.shape[1], y.shape[1]
    cost = torch.empty(F, device=x.device, dtype=torch.float32)
    iters = torch.empty(F, device=x.device, dtype=torch.int32)
    u = torch.empty(F, n, device=x.device, dtype=torch.float32) if want_potentials else None
    v = torch.empty(F, m, device=x.device, dtype=torch.float32) if want_potentials else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().piml_sinkhorn_frames(_ptr(x), _ptr(y), _ptr(mx), _ptr(my), F, n, m, float(eps), int(max_iter),
                                                   float(thresh), _ptr(cost), _ptr(iters), _ptr(u), _ptr(v), _stream()),
                   'piml_sinkhorn_frames')
    out = (cost.reshape(lead), iters.reshape(lead))
    if want_potentials:
        out += (u.reshape(*lead, n), v.reshape(*lead, m))
    return out


def mmd_frames(x, y, mask_x=None, mask_y=None, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """Multi-kernel Gaussian MMD of every frame (MaximumMeanDiscrepancy, src/functions/metrics.py:207-273, per frame),
    evaluated in float64: x (*c, n, 2), y (*c, m, 2), optional presence masks.  fix_sigma follows Python truthiness
    (None or 0: the bandwidth of the data).  Returns (*c) float32."""
    x, y, mx, my, lead = _pair(x, y, mask_x, mask_y)
    F, n, m = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty(F, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().piml_mmd_frames(_ptr(x), _ptr(y), _ptr(mx), _ptr(my), F, n, m, float(kernel_mul),
                                              int(kernel_num), float(fix_sigma) if fix_sigma else 0.0, _ptr(out), _stream()),
                   'piml_mmd_frames')
    return out.reshape(lead)
