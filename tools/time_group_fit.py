"""Measurements of the group side of the statistics fit (profiles/group_fit_summary.md): the group side of one
generation with the components on the host and on the device, a recovery run of Ag, and the fit on the recorded GC clip.

    python tools/time_group_fit.py [--out profiles/group_fit.json]"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from piml_amd import calibrate as C
from piml_amd.data.data import RawData
from piml_amd.groupstats import group_stats_of_raw, group_stats, host_rows
from piml_amd.models.mlapm import MLAPM
from piml_amd.scenarios import clip_scenario
from piml_amd.simulate import load_mlapm_params

GC = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else 'profiles/group_fit.json'
out = {}
raw = RawData()
raw.load_trajectory_data(GC)
T = int(raw.position.shape[0])
ref = group_stats_of_raw(raw)
out['recording'] = dict(frames=T, group_fraction=ref.group_fraction(), eligible=ref.eligible_tracks(), links=int(ref.links[0]),
                        mean_member_distance=ref.mean_member_distance(), size_tracks=ref.size_tracks[0].tolist())
print('recording', out['recording'], flush=True)
with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    scene = clip_scenario(raw, groups='auto').to('cuda:0')
law = load_mlapm_params(None)
print('law', law, flush=True)

# ---- 1. the group side of one generation: host against device, same process
cands = [dict(law, Ag=0.25 * c) for c in range(16)]
seeds = list(range(8))
res = {}
evs = {}
for comp in ('host', 'device'):
    ev = C._StatsEvaluator(scene, (None, None, None, ref), T, seeds, len(cands), 0.3, None, None, None, None, 50, 'cuda:0',
                           components=comp)
    evs[comp] = ev
    ev(cands)                                   # warm-up
    times, J = [], None
    for _ in range(3):
        before = dict(ev.seconds)
        J = ev(cands)
        times.append({k: ev.seconds[k] - before[k] for k in ev.seconds})
    res[comp] = dict(groups_ms=[1e3 * t['groups'] for t in times], run_ms=[1e3 * t['run'] for t in times],
                     host_ms=[1e3 * t['host'] for t in times], J=J)
    print(comp, res[comp], flush=True)
assert res['host']['J'] == res['device']['J']
out['generation'] = dict(members=len(cands) * len(seeds), frames=T, capacity=int(evs['host'].run.st.p.shape[-2]) if hasattr(evs['host'].run.st, 'p') else None, **res)
# host_rows alone on this generation's rows, and the kernel alone by events
sw = evs['device'].run.run(cands, 0.3)
n_active = [min(int(n), sw.capacity) for n in sw.spawned]
gs = group_stats(sw.position, sw.mask_p, n_active=n_active, dt=float(sw.time_unit), components='host')
rows = dict(edges=gs.edges, trk_steps=gs.trk_steps, trk_path=gs.trk_path)
t = []
for _ in range(3):
    t0 = time.perf_counter()
    host_rows(rows, gs.options['min_frames'], gs.options['share_q'])
    t.append(1e3 * (time.perf_counter() - t0))
out['generation']['host_rows_alone_ms'] = t
out['generation']['candidates_per_member'] = float(gs.candidates.mean())
out['generation']['links_per_member'] = float(gs.links.mean())
from piml_amd import ops_metrics
r2, dv2, vm2, mf, sq = ops_metrics.group_thresholds(float(sw.time_unit), 2.0, 0.5, 0.1, 2.0, 0.8)
pr = ops_metrics.group_pairs_frames(sw.position, sw.mask_p, r2, dv2, vm2, mf, None,
                                    torch.tensor(n_active, dtype=torch.int32, device='cuda:0'), int(gs.candidates.max()) + 1)
torch.cuda.synchronize()
kt = []
for _ in range(5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ops_metrics.group_components_frames(pr['edges'], pr['n_edges'], pr['trk_steps'], pr['trk_path'], mf, sq)
    b.record()
    torch.cuda.synchronize()
    kt.append(a.elapsed_time(b))
out['generation']['components_call_ms_events'] = kt
print(out['generation'], flush=True)
del evs, sw
with open(OUT, 'w') as fh:
    json.dump(out, fh, indent=1)

# ---- 2. a recovery run: reference simulated with Ag = 3 on 32 seeds, fitted from Ag = 1 on other seeds
ens = MLAPM(**law, Ag=3.0).simulate_ensemble(scene, T, list(range(100, 132)))
sim_ref = ens.group_stats(components='device').pooled()
del ens
init = {k: v for k, v in law.items() if k != 'version'}
t0 = time.perf_counter()
rec = C.calibrate_mlapm_to_stats(scene, (None, None, None, sim_ref), version=law['version'], init={**init, 'Ag': 1.0},
                                 fit=('Ag',), frames=T, seeds=range(8), population=16, generations=12)
out['recovery'] = dict(true_Ag=3.0, init_Ag=1.0, recovered_Ag=rec.params['Ag'], objective_before=rec.initial_loss,
                       objective_after=rec.final_loss, history=rec.history, terms=rec.terms, seconds=rec.seconds,
                       wall_s=time.perf_counter() - t0, ref_group_fraction=sim_ref.group_fraction())
print('recovery', out['recovery'], flush=True)
# the objective along Ag on the fit's seeds: how sharply is it identified?
ev = C._StatsEvaluator(scene, (None, None, None, sim_ref), T, list(range(8)), 16, 0.3, None, None, None, None, 50, 'cuda:0')
grid = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 2.75, 3.0, 3.25, 3.5, 4.0, 5.0, 6.0, 8.0, 12.0, 16.0]
out['recovery']['profile'] = dict(Ag=grid, J=ev([dict(law, Ag=g) for g in grid]))
print('profile', out['recovery']['profile'], flush=True)
with open(OUT, 'w') as fh:
    json.dump(out, fh, indent=1)

# ---- 3. the fit on the recorded clip itself (group side only), and the group fraction on held-out seeds
t0 = time.perf_counter()
fit = C.calibrate_mlapm_to_stats(scene, (None, None, None, ref), version=law['version'], init={**init, 'Ag': 3.0},
                                 fit=('Ag', 'group_dist'), frames=T, seeds=range(8), population=16, generations=12)
held = {}
for name, prm in (('fitted', fit.params), ('init Ag=3', dict(law, Ag=3.0)), ('no term', dict(law))):
    e = MLAPM(**prm).simulate_ensemble(scene, T, list(range(8, 16)))
    g = e.group_stats(components='device')
    J, terms = C.stats_objective(groups=g.pooled(), ref_groups=ref)
    held[name] = dict(group_fraction=g.group_fraction(), mean_member_distance=g.mean_member_distance(), J=J,
                      terms={k: terms[k] for k in C.OBJECTIVE_KEYS['groups']})
    del e
out['gc_fit'] = dict(Ag=fit.params['Ag'], group_dist=fit.params['group_dist'], objective_before=fit.initial_loss,
                     objective_after=fit.final_loss, history=fit.history, terms=fit.terms, held_out=held,
                     wall_s=time.perf_counter() - t0, seconds=fit.seconds)
print('gc_fit', out['gc_fit'], flush=True)
ev = C._StatsEvaluator(scene, (None, None, None, ref), T, list(range(8)), 16, 0.3, None, None, None, None, 50, 'cuda:0')
out['gc_fit']['profile'] = dict(Ag=grid, J=ev([dict(law, Ag=g) for g in grid]))
print('gc profile', out['gc_fit']['profile'], flush=True)
with open(OUT, 'w') as fh:
    json.dump(out, fh, indent=1, default=float)
print('done')
