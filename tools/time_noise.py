"""Time the MLAPM scenario frame with the fluctuation term beside the plain frame, fit the term to the recorded
GC clip's track statistics and record what it does to the GC ensemble's.

Frames: the GC scene (scenarios.SCENARIOS['gc']), --members seeds x --frames frames, main_mlapm.py's constants.  `plain` runs
the kernels of piml_scenario_step_mlapm, which the term leaves what they were (the yardstick); `noise` the same law with An,
noise_tau = --An, --noise-tau through piml_scenario_step_mlapm_noise.  Both captured (MLAPM.simulate_ensemble), by the method
of time_groups.py: per-frame cost = the difference of two runs of --frames and --short frames at one capacity (set-up,
capture and read-back cancel), each run between device synchronisations, --reps rounds after a warm-up, the two alternating
so that a busy neighbour hits both; the median and every round are kept.

Fit: calibrate --match-stats on the recorded GC clip (tests/golden) in the clip's own scene, --match crowd,pairs,tracks --fit
An,noise_tau --init An=0.5, --population candidates x seeds 0:8 x --generations generations.  It is judged on seeds the search
did not use (100:132): compare_track_stats of the clip scene's ensemble against the recording at An = 0 and at the fit.

Findings: the track statistics of the GC ensemble at An = 0 and at the fitted (An, noise_tau), next to the recorded GC clip's.

    python tools/time_noise.py [--reps 3] [--out profiles/noise_time.json] [--summary profiles/noise_summary.md]"""
import argparse
import json
import os
import sys
import tempfile

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from time_trackstats import finding  # noqa: E402

GC_CLIP = 'tests/golden/data/GC_Dataset_ped1-12685_time1000-1060_interp9_xrange5-25_yrange15-35.npy'
HELD_OUT = list(range(100, 132))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(res):
    t, fit = res['ms_per_frame'], res.get('fit')
    M = lambda k: f'{res["member_frames_per_s"][k] / 1e6:.2f} M'
    rows = ['# The fluctuation term (`piml_scenario_step_mlapm_noise`, DESIGN 4.29) on one MI355X', '',
            f'`python tools/time_noise.py --reps {res["reps"]}` (`noise_time.json`): the GC scene, {res["members"]} seeds x '
            f'{res["frames"][1]} frames, main_mlapm.py\'s constants, capacity {res["capacity"]}, captured; per-frame cost = the '
            f'difference of a {res["frames"][1]}- and a {res["frames"][0]}-frame run between device synchronisations, median of '
            f'{res["reps"]} rounds after a warm-up, the two runs alternating in one process.  `plain` runs the kernels of '
            '`piml_scenario_step_mlapm`, which the term leaves what they were on the parent commit.', '',
            '| frame | ms per frame (rounds) | member-frames / s | against |', '|---|---|---|---|',
            f'| plain | {t["plain"]} ({", ".join(str(x) for x in res["ms_per_frame_rounds"]["plain"])}) | {M("plain")} | |',
            f'| An = {res["noise"]["An"]}, noise_tau = {res["noise"]["noise_tau"]} | {t["noise"]} '
            f'({", ".join(str(x) for x in res["ms_per_frame_rounds"]["noise"])}) | {M("noise")} | {res["noise_over_plain"]} x plain |',
            '', 'The term is one Philox call and two double-precision Box-Muller normals on one lane per live agent, one 8-byte '
            'read and write of its state, a broadcast and two adds.  Kernel times were not traced.', '']
    if fit:
        rows += [f'Fit (`fit` in `noise_time.json`): `calibrate --match-stats --match {",".join(fit["match"])} --fit An,noise_tau '
                 f'--init An={fit["init_An"]}` on the recorded GC clip in its own scene, {fit["population"]} candidates x seeds '
                 f'0:{fit["seeds"]} x {fit["generations"]} generations: objective {fit["initial_loss"]:.4g} -> '
                 f'{fit["final_loss"]:.4g} ({fit["status"]}), An = {fit["An"]:.4g} m/s^2, noise_tau = {fit["noise_tau"]:.4g} s.  '
                 f'On seeds the search did not use ({HELD_OUT[0]}:{HELD_OUT[-1] + 1}), the clip scene\'s ensemble against the '
                 'recording (`compare_track_stats`, `min_count` 50):', '',
                 '| term | An = 0 | fitted |', '|---|---|---|']
        for k in fit['held_out']['zero']:
            rows.append(f'| {k} | {fit["held_out"]["zero"][k]} | {fit["held_out"]["fitted"][k]} |')
        rows += ['', 'The objective\'s first value is the init\'s (An = 0.5, white noise), not the law without the term; the crowd and '
                 'pair terms are in it too.  Not measured: the fit\'s spread over search seeds, the UCY clip, any scene but these two.',
                 '']
    if 'findings' in res:
        rows += ['Findings (`findings` in `noise_time.json`, `min_count` 50; recorded, not asserted):', '',
                 '| crowd | persistence time s | MSD exponent | mean acceleration m/s^2 | mean straightness (complete) | '
                 'tracks (complete) | A(tau) |', '|---|---|---|---|---|---|---|']
        for k, v in res['findings'].items():
            rows.append(f'| {k} | {v["persistence_time_s"]} | {v["msd_exponent"]} | {v["mean_acceleration"]} | '
                        f'{v["mean_straightness"]} ({v["mean_straightness_complete"]}) | {v["tracks"]} '
                        f'({v["complete_tracks"]}) | {v["A"]} |')
    return '\n'.join(rows) + '\n'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--frames', type=int, default=750)
    ap.add_argument('--short', type=int, default=150)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--An', type=float, default=0.5)
    ap.add_argument('--noise-tau', dest='noise_tau', type=float, default=0.5)
    ap.add_argument('--population', type=int, default=16)
    ap.add_argument('--generations', type=int, default=20)
    ap.add_argument('--no-fit', dest='fit', action='store_false')
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--summary', type=str, default=None)
    a = ap.parse_args(argv)
    from piml_amd import _lib, calibrate
    from piml_amd.calibrate import DEFAULT_INIT
    from piml_amd.data.data import RawData
    from piml_amd.models.mlapm import MLAPM
    from piml_amd.scenarios import SCENARIOS, clip_scenario, default_capacity
    from piml_amd.trackstats import compare_track_stats, track_stats_of_raw
    gc = SCENARIOS['gc']().to('cuda:0')
    cap = default_capacity(gc, a.frames)
    runs = {'plain': MLAPM(version='GC', **DEFAULT_INIT),
            'noise': MLAPM(version='GC', **DEFAULT_INIT, An=a.An, noise_tau=a.noise_tau)}
    usage = _lib.kernel_resource_usage()
    S = a.members
    seeds = list(range(S))
    res = {'frames': [a.short, a.frames], 'reps': a.reps, 'members': S, 'capacity': cap,
           'noise': {'An': a.An, 'noise_tau': a.noise_tau},
           'kernels': {k: {f: v[f] for f in ('vgprs', 'agprs', 'vgpr_spill', 'scratch_bytes', 'lds_bytes')}
                       for k, v in usage.items() if k.startswith(('noise_force', 'scenario_mlapm_noise', 'scenario_mlapm_kernel'))},
           'ms_per_frame': {}, 'ms_per_frame_rounds': {}, 'member_frames_per_s': {}}
    med = lambda x: sorted(x)[len(x) // 2]
    run = lambda k, T: timed(lambda: runs[k].simulate_ensemble(gc, T, seeds, capacity=cap))
    per = {k: [] for k in runs}
    for k in runs:                                           # warm-up of both at the timed shapes
        run(k, a.short)
    for _ in range(a.reps):                                  # the two alternate
        for k in runs:
            per[k].append((run(k, a.frames) - run(k, a.short)) / (a.frames - a.short))
    for k in runs:
        ms = med(per[k])
        res['ms_per_frame'][k] = round(ms, 5)
        res['ms_per_frame_rounds'][k] = [round(x, 5) for x in per[k]]
        res['member_frames_per_s'][k] = round(S / ms * 1e3, 1)
    res['noise_over_plain'] = round(res['ms_per_frame']['noise'] / res['ms_per_frame']['plain'], 4)
    print(f'[noise] GC scene, S={S}: ms per frame {res["ms_per_frame"]}, member-frames/s {res["member_frames_per_s"]}', flush=True)

    raw = RawData()
    raw.load_trajectory_data(os.path.join(ROOT, GC_CLIP))
    rec = track_stats_of_raw(raw)
    fitted = None
    if a.fit:
        match = ('crowd', 'pairs', 'tracks')
        with tempfile.TemporaryDirectory() as tmp:
            out = calibrate.main(['--data', os.path.join(ROOT, GC_CLIP), '--match-stats', '--match', ','.join(match), '--fit',
                                  'An,noise_tau', '--init', 'An=0.5', '--seeds', '0:8', '--population', str(a.population),
                                  '--generations', str(a.generations), '--out', os.path.join(tmp, 'params.json')])
        fitted = {k: out.params[k] for k in ('An', 'noise_tau')}
        rnd = lambda d: {k: (None if v != v else round(float(v), 4)) if isinstance(v, float) else v for k, v in d.items()}
        scene = clip_scenario(raw).to('cuda:0')
        held = {}
        for tag, extra in (('zero', {}), ('fitted', fitted)):
            ens = MLAPM(version='GC', **DEFAULT_INIT, **extra).simulate_ensemble(scene, raw.num_steps, HELD_OUT)
            held[tag] = rnd(compare_track_stats(ens.track_stats(), rec, 50))
        res['fit'] = dict(match=list(match), init_An=0.5, population=a.population, generations=a.generations, seeds=8,
                          initial_loss=out.initial_loss, final_loss=out.final_loss, status=out.status, history=out.history,
                          terms=rnd(out.terms or {}), seconds=out.seconds, held_out=held, **fitted)
        print(f'[noise] fit: {res["fit"]}', flush=True)
    f = {'recorded_gc_clip': finding(rec)}
    f[f'mlapm_gc_ensemble_{S}x{a.frames}_An0'] = finding(runs['plain'].simulate_ensemble(gc, a.frames, seeds, capacity=cap).track_stats())
    if fitted is not None:
        law = MLAPM(version='GC', **DEFAULT_INIT, **fitted)
        f[f'mlapm_gc_ensemble_{S}x{a.frames}_fitted'] = finding(law.simulate_ensemble(gc, a.frames, seeds, capacity=cap).track_stats())
    for k, v in f.items():
        print(f'[noise] {k}: {v}', flush=True)
    res['findings'] = f
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    if a.summary:
        with open(a.summary, 'w') as fh:
            fh.write(summary(res))
    print(json.dumps({k: v for k, v in res.items() if k not in ('findings', 'kernels')}))


if __name__ == '__main__':
    main()
