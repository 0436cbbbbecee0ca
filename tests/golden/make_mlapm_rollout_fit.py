"""Fixture of the MLAPM rollout calibration loss (tests/test_mlapm_rollout_fit_gpu.py): H closed-loop steps of the
reference's own `models.mlapm.MLAPM.step` per window in float64, differentiated by autograd with respect to its six
constants, on 12 windows of the GC test clip.

    python tests/golden/make_mlapm_rollout_fit.py <reference checkout>   (writes tests/golden/mlapm_rollout_fit.npz, CPU only)

A window starts at t0 = 300, 303, ..., 333 and runs H = 8 steps.  S_k = the agents present in frame t0 + k (finite p, v,
destination and mask_v != 0).  At k = 0 every agent of S_0 takes its recorded (p, v); step k computes MLAPM.step over
S_k on the simulated states with the recorded destinations of frame t0 + k, then p' = p + v' dt (main_mlapm.py:25).
Agents of S_{k+1} that were in S_k keep the simulated state; those that were not enter with their recorded state (the
reference's new_peds_flag) and carry no gradient.  The loss is sum w_k |p^_k - P_k|^2 / sum w_k over the (k >= 1, agent)
whose state was carried, w_k = time_decay^(H - k).  Desired speed: the mean |v| over the first 25 frames after the agent
starts moving.  Variants raw and GC (the reference's UCY branch raises for more than two agents), two parameter points,
time_decay 1 and 0.9.  Besides loss and gradient: the per-constant scale sum_windows |d numerator_w / d constant| / sum w
(the gradient is a sum with cancellations), the term count, and the per-step squared-error sums and counts.
No reference source is copied: the reference is imported and called."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CLIP = os.path.join(HERE, 'data', 'GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy')
H, STRIDE, FIRST, WINDOWS = 8, 3, 300, 12
NAMES = ('tau', 'A', 'B', 'C', 'D', 'theta')
POINTS = ({'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0},      # src/main_mlapm.py:16
          {'tau': 0.8, 'A': 4.0, 'B': -1.5, 'C': 0.6, 'D': -0.1, 'theta': 25.0})
DECAYS = (1.0, 0.9)
RADIUS = 0.3


def window(model, P, V, D, present, v0, t0, dt, decay):
    """(weighted numerator, weight, per-step sse (H), per-step count (H)) of one window, under autograd."""
    N = P.shape[1]
    p = torch.tensor(np.nan_to_num(P[t0]))
    v = torch.tensor(np.nan_to_num(V[t0]))
    num = torch.zeros((), dtype=torch.float64)
    wsum, sse, cnt = 0.0, np.zeros(H), np.zeros(H)
    for k in range(H):
        t = t0 + k
        idx = np.nonzero(present[t])[0]
        vn = model.step(p[idx], v[idx], torch.tensor(v0[idx, None]), torch.tensor(D[t, idx]), dt=dt, radius=RADIUS)
        carried = present[t] & present[t + 1]
        vfull = torch.zeros(N, 2, dtype=torch.float64).index_copy(0, torch.tensor(idx), vn)
        pfull = torch.zeros(N, 2, dtype=torch.float64).index_copy(0, torch.tensor(idx), p[idx] + vn * dt)
        c = torch.tensor(carried)[:, None]
        p = torch.where(c, pfull, torch.tensor(np.nan_to_num(P[t + 1])))
        v = torch.where(c, vfull, torch.tensor(np.nan_to_num(V[t + 1])))
        w = decay ** (H - (k + 1))
        ci = np.nonzero(carried)[0]
        e2 = ((p[ci] - torch.tensor(P[t + 1, ci])) ** 2).sum(-1)
        num = num + w * e2.sum()
        wsum += w * len(ci)
        sse[k] = float(e2.sum())
        cnt[k] = len(ci)
    return num, wsum, sse, cnt


def main(ref):
    sys.path.insert(0, os.path.join(ref, 'src'))
    sys.path.insert(0, REPO)
    from models.mlapm import MLAPM                       # the reference's class
    from piml_amd.data.data import RawData
    raw = RawData()
    raw.load_trajectory_data(CLIP)
    P, V, D = (x.numpy().astype(np.float64) for x in (raw.position, raw.velocity, raw.destination))
    present = np.isfinite(P).all(-1) & np.isfinite(V).all(-1) & np.isfinite(D).all(-1) & (raw.mask_v.numpy() != 0)
    T, N = present.shape
    speed = np.linalg.norm(np.where(present[..., None], V, 0.0), axis=-1)
    v0 = np.zeros(N)
    for n in range(N):
        mv = np.nonzero(speed[:, n] > 0)[0]
        if len(mv):
            v0[n] = speed[mv[0]:mv[0] + 25, n].mean()
    dt = float(raw.time_unit)
    starts = [FIRST + STRIDE * w for w in range(WINDOWS)]
    out = {'frames': np.array([FIRST, starts[-1] + H + 1]), 'stride': STRIDE, 'horizon': H, 'starts': np.array(starts),
           'names': np.array(NAMES), 'radius': RADIUS, 'dt': dt, 'decays': np.array(DECAYS)}
    for version in ('raw', 'GC'):
        for k, point in enumerate(POINTS):
            for q, decay in enumerate(DECAYS):
                prm = {n: torch.tensor(point[n], dtype=torch.float64, requires_grad=True) for n in NAMES}
                model = MLAPM(version=version, **prm)
                nums, wsum, jac, sse, cnt = [], 0.0, [], np.zeros(H), np.zeros(H)
                for t0 in starts:
                    num, w, s, c = window(model, P, V, D, present, v0, t0, dt, decay)
                    g = torch.autograd.grad(num, [prm[n] for n in NAMES], allow_unused=True)
                    jac.append([0.0 if x is None else float(x) for x in g])
                    nums.append(float(num))
                    wsum += w
                    sse += s
                    cnt += c
                J = np.array(jac)
                tag = f'{version}_{k}_{q}'
                out[f'params_{tag}'] = np.array([point[n] for n in NAMES])
                out[f'loss_{tag}'] = sum(nums) / wsum
                out[f'grad_{tag}'] = J.sum(0) / wsum
                out[f'grad_scale_{tag}'] = np.abs(J).sum(0) / wsum
                out[f'count_{tag}'] = int(cnt.sum())
                out[f'sse_{tag}'] = sse
                out[f'step_count_{tag}'] = cnt
                print(tag, out[f'loss_{tag}'], out[f'grad_{tag}'], out[f'grad_scale_{tag}'], out[f'count_{tag}'])
    np.savez(os.path.join(HERE, 'mlapm_rollout_fit.npz'), **out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
