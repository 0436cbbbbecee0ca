"""MLAPM's backward entry points through the C ABI, shared by the GPU test files."""
import numpy as np
import torch

DEV = 'cuda:0'


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


_LAWS = dict(raw=dict(tau=0.5, A=7.55, B=-3.0), GC=dict(tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56),
             UCY=dict(tau=5 / 6, A=10.67, B=-3.33, C=0.5, theta=20))


def _mlapm_bwd_direct(entry, sc, w, ver, workspace=None, law=None):
    """piml_mlapm_step_bwd / piml_mlapm_step_bwd_ws through the C ABI on the same inputs (law: constants other than
    _LAWS[ver]'s)"""
    from piml_amd import _lib, ops
    pr = dict(C=0.0, D=0.0, theta=0.0)
    pr.update(_LAWS[ver] if law is None else law)
    p, v, v0, d = [dev(sc[k]) for k in ('position', 'velocity', 'desired_speed', 'destination')]
    N = p.shape[0]
    out = [torch.full((N, 2), float('nan'), device=DEV), torch.full((N, 2), float('nan'), device=DEV),
           torch.full((N,), float('nan'), device=DEV), torch.full((N, 2), float('nan'), device=DEV)]
    ptr = lambda t: t.data_ptr()
    args = [ptr(w), ptr(p), ptr(v), ptr(v0), ptr(d), N, ops.MLAPM_VARIANTS[ver], pr['tau'], pr['A'], pr['B'], pr['C'], pr['D'],
            pr['theta'], 0.3, 0.08, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])]
    L = _lib.lib()
    if entry == 'ws':
        need = int(L.piml_mlapm_bwd_workspace_floats(N, ops.MLAPM_VARIANTS[ver]))
        assert need > 0
        ws = torch.full((need,), float('nan'), device=DEV) if workspace is None else workspace
        rc = L.piml_mlapm_step_bwd_ws(*args, ptr(ws), ws.numel(), None)
    else:
        rc = L.piml_mlapm_step_bwd(*args, None)
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in out]
