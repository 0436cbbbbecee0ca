"""Time piml_pair_stats and record the g(tau) findings.

Timing: GC ensembles of S = 1 / 8 / 32 members x 750 frames at the default capacity (crowds from the MLAPM law, which is
cheap to simulate; the statistics do not care what drove them), with and without the GC box, and the recorded GC clip, all
with the default options (R = 0.5 m, lags 64 / 128 / 192).  Device time per call from events around `reps` back-to-back
calls of ops_metrics.pair_stats_frames (a memset and two launches); end to end = pairstats.pair_stats with its read-back,
from a host clock.  Pair evaluations = the device's own `pairs` count summed over the lags (ordered pairs evaluated).

Findings: g(tau), E(tau) and the energy exponent of the recorded GC (GC box) and UCY clips and of 8-member GC ensembles
driven by MLAPM (main_mlapm.py's constants) and by a PINNSF (pinnsf_m with its seeded initial weights: no trained
checkpoint ships with the project).

    python tools/time_pairstats.py [--reps 20] [--out profiles/pairstats_time.json]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CLIPS = {'gc': 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy',
         'ucy': 'tests/golden/data/UCY_Dataset_time162-216_timeunit0.08.npy'}
BOX = (5.0, 25.0, 15.0, 35.0)
LAGS = (64, 128, 192)


def time_one(P, V, M, n_active, box, reps):
    from piml_amd import ops_metrics, pairstats
    na = None if n_active is None else torch.tensor(n_active, device=P.device, dtype=torch.int32)
    args = (P, V, M, 0.5, LAGS, 0.1, 100, 0.05, 100, None, box, None, na)
    for _ in range(3):
        out = ops_metrics.pair_stats_frames(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops_metrics.pair_stats_frames(*args)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / reps
    t = time.perf_counter()
    for _ in range(reps):
        pairstats.pair_stats(P, V, M, box=box, n_active=n_active)
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t) * 1e3 / reps
    pairs = int(out['pairs'].sum().item())
    return dict(device_ms=round(dev_ms, 4), end_to_end_ms=round(e2e_ms, 4), pair_evaluations=pairs,
                focal_agent_frames_lag0=int(out['focal'][:, 0].sum().item()),
                pair_evaluations_per_s=float(f'{pairs / (dev_ms * 1e-3):.4g}'))


def finding(st):
    p, n = st.energy_exponent()
    g = st.g_tau()
    e = st.interaction_energy()
    tau = st.tau_centres
    ok = np.isfinite(g)
    return dict(energy_exponent=None if not np.isfinite(p) else round(p, 4), energy_bins=n,
                overlap_rate=round(st.overlap_rate(), 6), focal_agent_frames=int(st.pooled().focal[0, 0]),
                g_tau={f'{tau[k]:.2f}': round(float(g[k]), 4) for k in np.nonzero(ok)[0][:30]},
                energy={f'{tau[k]:.2f}': round(float(e[k]), 4) for k in np.nonzero(ok)[0][:30]})


def _pinnsf():
    from piml_amd.models.simulators import BaseSimulator
    a = types.SimpleNamespace(
        ped_feature_dim=6, obs_feature_dim=6, self_feature_dim=7, encoder_hidden_size=128, processor_hidden_size=128,
        decoder_hidden_size=64, encoder_hidden_layers=3, processor_hidden_layers=16, decoder_hidden_layers=2, dropout=0.5,
        activation='relu', dataset_name='gc1560', res_hidden_layers=3, model='pinnsf_m', device='cuda:0', gpus='0',
        learning_rate=0.002, weight_decay=5e-4, batch_size=3, topk_ped=6, topk_obs=10, sight_angle_ped=90,
        sight_angle_obs=90, dist_threshold_ped=4, dist_threshold_obs=4, num_history_velocity=1, skip_frames=25,
        valid_steps=5, time_decay=1, reg_weight=0., collision_threshold=0.5, collision_loss_weight=10,
        val_coll_weight=30, hard_collision_penalty=10, teacher_weight=0, collision_pred_weight=10,
        collision_focus_weight=10, new_collision_loss_flag=0, collision_loss_version='v0', finetune_lr_decay=1,
        finetune_wd_aug=1, ft_lr_decay2=0., exp_name='pairstats', model_name_suffix='x', epochs=1, patience=1,
        ft_patience=5, pinnsf_interaction='sim', iter_flag=0, true_label_weight=0)
    torch.manual_seed(0)
    sim = BaseSimulator(a)
    sim.model.eval()
    return sim


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--members', type=str, default='1,8,32')
    ap.add_argument('--no-findings', dest='findings', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.pairstats import pair_stats_of_raw
    from piml_amd.scenarios import SCENARIOS
    sc = SCENARIOS['gc']().to('cuda')
    law = MLAPM(version='GC', tau=0.5, A=7.55, B=-3.0, C=0.2, D=-0.3, theta=56.0)
    res = {'frames': 750, 'reps': a.reps, 'radius': 0.5, 'lags': list(LAGS), 'tau_bins': 100, 'r_bins': 100, 'gc': {}}
    for S in (int(s) for s in a.members.split(',')):
        ens = law.simulate_ensemble(sc, 750, list(range(S)))
        cap = ens.position.shape[2]
        n_active = [min(int(n), cap) for n in ens.spawned]
        res['capacity'] = cap
        for tag, box in (('no_box', None), ('box', BOX)):
            r = time_one(ens.position, ens.velocity, ens.mask_p, n_active, box, a.reps)
            res['gc'].setdefault(str(S), {})[tag] = r
            print(f'[pairstats] GC S={S} x 750 frames, cap {cap}, {tag}: {r}', flush=True)
        del ens
    raws = {}
    for k, path in CLIPS.items():
        raws[k] = RawData()
        raws[k].load_trajectory_data(os.path.join(ROOT, path))
    raw = raws['gc']
    dev = lambda x: x.to('cuda').contiguous()
    r = time_one(dev(raw.position)[None], dev(raw.velocity)[None], dev(raw.mask_p)[None], None, BOX, a.reps)
    res['recorded_gc_clip'] = dict(frames=raw.num_steps, agents=raw.num_pedestrians, **r)
    print(f'[pairstats] recorded GC clip ({raw.num_steps} frames, {raw.num_pedestrians} agents), box: {r}', flush=True)
    if a.findings:
        f = {}
        f['recorded_gc_clip_box'] = finding(pair_stats_of_raw(raws['gc'], box=BOX))
        f['recorded_ucy_clip'] = finding(pair_stats_of_raw(raws['ucy']))
        f['mlapm_gc_ensemble_8x750_box'] = finding(law.simulate_ensemble(sc, 750, list(range(8))).pair_stats(box=BOX))
        f['pinnsf_initial_weights_gc_ensemble_8x750_box'] = finding(
            _pinnsf().simulate_ensemble(sc, 750, list(range(8))).pair_stats(box=BOX))
        for k, v in f.items():
            print(f'[pairstats] {k}: exponent {v["energy_exponent"]} over {v["energy_bins"]} bins, overlap rate '
                  f'{v["overlap_rate"]}, g(tau) {v["g_tau"]}', flush=True)
        res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'findings'}))


if __name__ == '__main__':
    main()
