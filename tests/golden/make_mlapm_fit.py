"""Fixture of the MLAPM calibration loss (tests/test_mlapm_fit_gpu.py): the reference's own `models.mlapm.MLAPM.step`
in float64, differentiated by autograd with respect to its six constants, on 40 frames of the GC test clip.

    python tests/golden/make_mlapm_fit.py <reference checkout>        (writes tests/golden/mlapm_fit.npz, CPU only)

Each frame is compacted to its present agents, as src/main_mlapm.py does before every step: an agent is present in
frame t when the clip lists it there with a velocity (the loader's mask_v; an agent's last frame has none).  The target
of a present agent is its velocity in frame t + 1 when it is present then; the loss is the mean over those agents of
|step(frame t)_i - target_i|^2.  Desired speed: the mean |v| over the first 25 frames after the agent starts moving.
Variants raw and GC (the reference's UCY branch raises for more than two agents).  Besides loss and gradient, every
quantity's scale is stored: the mean over agents of |d loss_i / d constant| (the gradient is a sum with cancellations).
No reference source is copied: the reference is imported and called."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CLIP = os.path.join(HERE, 'data', 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy')
FRAMES = list(range(300, 340))
NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
POINTS = ({'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0},      # src/main_mlapm.py:16
          {'tau': 0.8, 'A': 4.0, 'B': -1.5, 'C': 0.6, 'D': -0.1, 'theta': 25.0})
RADIUS = 0.3


def main(ref):
    sys.path.insert(0, os.path.join(ref, 'src'))
    sys.path.insert(0, REPO)
    from models.mlapm import MLAPM                       # the reference's class
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(CLIP)
    P, V, D = (x.numpy().astype(np.float64) for x in (raw.position, raw.velocity, raw.destination))
    present = np.isfinite(P).all(-1) & (raw.mask_v.numpy() != 0)
    T, N = present.shape
    speed = np.linalg.norm(np.where(present[..., None], V, 0.0), axis=-1)
    v0 = np.zeros(N)
    for n in range(N):
        mv = np.nonzero(speed[:, n] > 0)[0]
        if len(mv):
            v0[n] = speed[mv[0]:mv[0] + 25, n].mean()
    dt = float(raw.time_unit)
    out = {'frames': np.array(FRAMES), 'names': np.array(NAMES), 'radius': RADIUS, 'dt': dt}
    for version in ('raw', 'GC'):
        for k, point in enumerate(POINTS):
            prm = {n: torch.tensor(point[n], dtype=torch.float64, requires_grad=True) for n in NAMES}
            model = MLAPM(version=version, **prm)
            losses, jac = [], []
            for t in FRAMES:
                idx = np.nonzero(present[t])[0]
                focal = present[t + 1, idx]
                if not focal.any():
                    continue
                pred = model.step(torch.tensor(P[t, idx]), torch.tensor(V[t, idx]), torch.tensor(v0[idx, None]),
                                  torch.tensor(D[t, idx]), dt=dt, radius=RADIUS)
                res = pred[torch.tensor(focal)] - torch.tensor(V[t + 1, idx[focal]])
                li = (res ** 2).sum(-1)
                for i in range(li.shape[0]):
                    g = torch.autograd.grad(li[i], [prm[n] for n in NAMES], retain_graph=True, allow_unused=True)
                    jac.append([0.0 if x is None else float(x) for x in g])
                losses.append(li.detach())
            li = torch.cat(losses)
            J = np.array(jac)
            tag = f'{version}_{k}'
            out[f'params_{tag}'] = np.array([point[n] for n in NAMES])
            out[f'loss_{tag}'] = float(li.mean())
            out[f'grad_{tag}'] = J.mean(0)
            out[f'grad_scale_{tag}'] = np.abs(J).mean(0)
            out[f'count_{tag}'] = li.shape[0]
            print(tag, out[f'loss_{tag}'], out[f'grad_{tag}'], out[f'grad_scale_{tag}'])
    np.savez(os.path.join(HERE, 'mlapm_fit.npz'), **out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
