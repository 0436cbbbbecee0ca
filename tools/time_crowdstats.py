"""Time piml_crowd_stats: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity
(the crowds come from the MLAPM law, which is cheap to simulate; the statistics do not care what drove them) and the
recorded GC clip.  Device time per call from events around `reps` back-to-back calls of ops_metrics.crowd_stats_frames
(two launches and a memset); the end-to-end time of crowdstats.crowd_stats (with its read-back) from a host clock.  Pair
terms = sum over slices of (focal agents x present agents), what the density pass must evaluate.
--density voronoi times piml_crowd_stats_voronoi (cutoff 1.0, the box as the walkable area where there is a
box) and the Gaussian call in the same run, the two alternating `--repeats` times: every figure is the median of the
repeats, with their smallest and largest value as the run-to-run spread.

    python tools/time_crowdstats.py [--reps 20] [--out profiles/crowdstats_time.json]
    python tools/time_crowdstats.py --density voronoi [--repeats 5] [--out profiles/voronoi_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
BOX = (5.0, 25.0, 15.0, 35.0)


def pair_terms(P, M, n_active, box):
    pres = (M == 1) & torch.isfinite(P).all(-1)
    if n_active is not None:
        slot = torch.arange(P.shape[2], device=P.device)
        pres &= slot[None, None, :] < torch.as_tensor(n_active, device=P.device)[:, None, None]
    focal = pres
    if box is not None:
        x, y = P[..., 0], P[..., 1]
        focal = pres & (x >= BOX[0]) & (x < BOX[1]) & (y >= BOX[2]) & (y < BOX[3])
    return int((focal.sum(-1).double() * pres.sum(-1).double()).sum().item())


def time_one(P, V, M, n_active, box, reps, density='gaussian'):
    from piml_amd import crowdstats, ops_metrics
    grid = None if box is None else crowdstats.grid_shape(box, 0.5)
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    if density == 'voronoi':
        dirs = crowdstats.voronoi_dirs()
        call = lambda: ops_metrics.crowd_stats_voronoi_frames(P, V, M, 1.0, dirs, box, box, grid, 0.5, 0.25, 24, None, False, na)
        kw = dict(density='voronoi', bounds=box)
    else:
        call = lambda: ops_metrics.crowd_stats_frames(P, V, M, 0.7, box, grid, 0.5, 0.25, 24, None, False, na)
        kw = {}
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / reps
    t = time.perf_counter()
    for _ in range(reps):
        crowdstats.crowd_stats(P, V, M, box=box, n_active=n_active, **kw)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / reps
    pairs = pair_terms(P, M, n_active, box)
    return dict(device_ms=round(dev_ms, 4), end_to_end_ms=round(e2e_ms, 4), pair_terms=pairs,
                pair_terms_per_s=float(f'{pairs / (dev_ms * 1e-3):.4g}'))


def time_both(P, V, M, n_active, box, reps, repeats):
    """Gaussian and Voronoi alternating `repeats` times: {density: time_one's dict with medians, and the spread}."""
    runs = {'gaussian': [], 'voronoi': []}
    for _ in range(repeats):
        for density in runs:
            runs[density].append(time_one(P, V, M, n_active, box, reps, density))
    out = {}
    for density, rs in runs.items():
        med = lambda k: sorted(r[k] for r in rs)[len(rs) // 2]
        out[density] = dict(device_ms=med('device_ms'), end_to_end_ms=med('end_to_end_ms'),
                            device_ms_spread=[min(r['device_ms'] for r in rs), max(r['device_ms'] for r in rs)],
                            pair_terms=rs[0]['pair_terms'])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--members', type=str, default='1,8,32')
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--density', choices=('gaussian', 'voronoi'), default='gaussian')
    ap.add_argument('--repeats', type=int, default=5, help='--density voronoi: alternating repeats of the two calls')
    a = ap.parse_args(argv)
    one = (lambda *x: time_both(*x, a.repeats)) if a.density == 'voronoi' else time_one
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS
    from piml_amd.data.data import RawData
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    res = {'frames': 750, 'reps': a.reps, 'radius': 0.7, 'rho_bins': 24, 'gc': {}}
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        n_active = [min(int(n), cap) for n in ens.spawned]
        res['capacity'] = cap
        for tag, box in (('no_box', None), ('box', BOX)):
            r = one(ens.position, ens.velocity, ens.mask_p, n_active, box, a.reps)
            res['gc'].setdefault(str(S), {})[tag] = r
            print(f'[crowdstats] GC S={S} x 750 frames, cap {cap}, {tag}: {r}', flush=True)
        del ens
    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    dev = lambda x: x.to('cuda').contiguous()
    r = one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, BOX, a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    if a.density == 'voronoi':
        from piml_amd import _lib
        usage = _lib.kernel_resource_usage()
        res.update(density='voronoi', cutoff=1.0, sides=16, repeats=a.repeats,
                   kernels={k: usage[k] for k in ('voronoi_cell_kernel', 'crowd_given_density_kernel', 'crowd_density_kernel')
                            if k in usage})
    print(f'[crowdstats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents), box: {r}', flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
