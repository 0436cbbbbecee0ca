"""Per-wave work statistics and in-kernel phase stamps of relfeat fwd from the -DPIML_RELFEAT_STATS
build (development aid; the stamps perturb the kernel, read shares not totals).  With the step's deferred weight pack in the launch
(PIML_DEFER_PACK), per form of piml_relfeat_pack_form: where the pack blocks start and end against the pedestrian passes."""
import sys, os, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import numpy as np
from piml_amd import _lib
# run with PIML_LIB=piml_amd/libpiml_hip_stats.so (python -m piml_amd.build --variant stats relfeat.hip:-DPIML_RELFEAT_STATS)
from piml_amd import ops
from piml_amd.scenes import synthetic_gc_scene
import piml_amd.models.model as MODEL

L = _lib.lib()
dev = 'cuda:0'
margs = types.SimpleNamespace(
    ped_feature_dim=6, obs_feature_dim=6, self_feature_dim=7, encoder_hidden_size=128, processor_hidden_size=128,
    decoder_hidden_size=64, encoder_hidden_layers=3, processor_hidden_layers=16, decoder_hidden_layers=2, dropout=0.5,
    activation='relu', dataset_name='ucy', res_hidden_layers=3, correction_hidden_layers=1, time_unit=0.08, collision_threshold=0.5)
torch.manual_seed(0)
model = MODEL.PINNSF_multitask(margs).to(dev).eval()
model.messages_wanted = False                       # the benchmarked step's pack: plain images + the folded ones
spec, fold = model._pack_spec(), model._fold_spec()
packs = ops.PinnsfPacks()
PACK_SLOTS = 4096                                   # pack-block records behind the rows' (4 ints each; no pack has this many blocks)


def rel(x, ref):
    """stamps are the low 32 bits of the counter: differences against `ref` as signed 32-bit numbers"""
    return ((x.astype(np.int64) - int(ref) + (1 << 31)) % (1 << 32)) - (1 << 31)


for N, M in ((4096, 2000),):
    sc = synthetic_gc_scene(N, M, seed=0)
    t = [torch.tensor(sc[k], device=dev) for k in ('position', 'velocity', 'acceleration', 'destination', 'obstacles')]
    alive = ~np.isnan(sc['position'][:, 0])
    for form in (None, 0, 1):
        # split launches: the obstacle workgroups' rows in the second half; the pack blocks' records behind them
        stats = torch.zeros(2 * N * 12 + PACK_SLOTS * 4, dtype=torch.int32, device=dev)
        os.environ['PIML_RELFEAT_STATS_PTR'] = str(stats.data_ptr())
        if form is not None:
            L.piml_relfeat_pack_form(form)
        for _ in range(3):
            stats.zero_()
            if form is not None:
                ops.pinnsf_prepack(packs, *spec, defer=True, fold=fold)
            ops.relative_features(*t)
        torch.cuda.synchronize()
        flat = stats.cpu().numpy()
        s2, pk = flat[:2 * N * 12].reshape(2 * N, 12), flat[2 * N * 12:].reshape(PACK_SLOTS, 4)
        s = s2[:N]
        print(f'== N={N} M={M}: ' + ('no pack in the launch' if form is None else f'deferred pack, form {form} ({("trailing workgroups", "obstacle workgroups tail")[form]})'))
        if form is None:
            for q, name in enumerate(('evals', 'drain rounds', 'insertions', 'candidates')):
                print(f'N={N} {name:13s}: mean {s[alive, q].mean():7.2f}  p50 {np.percentile(s[alive, q], 50):6.0f}  p99 {np.percentile(s[alive, q], 99):6.0f}  max {s[alive, q].max():6d}')
        names = ['entry->ped tile staged', 'ped pass', 'obs tile staged (incl. barrier wait)', 'obs pass']
        st = s[alive, 4:9].astype(np.int64)
        split = bool(s2[N:].any())
        for q, name in enumerate(names[:2] if split else names):
            dphase = st[:, q + 1] - st[:, q]
            print(f'  phase {name:38s}: median {np.median(dphase):8.0f} cycles  p90 {np.percentile(dphase, 90):8.0f}  max {dphase.max():8d}')
        if split:
            print('  split launch: the rows above are the pedestrian workgroups (entry, staged, pass done); obstacle workgroups:')
            so = s2[N:][alive, 4:9].astype(np.int64)
            for q, name in enumerate(('entry->obs tile staged', 'obs pass')):
                d = so[:, q + 1] - so[:, q]
                print(f'  phase {name:38s}: median {np.median(d):8.0f} cycles  p90 {np.percentile(d, 90):8.0f}  max {d.max():8d}')
        else:
            print('  total to end of obs pass: median', np.median(st[:, 4]), 'cycles')
        # absolute times on the device's 100 MHz clock (slots 9 / 10: a wave's entry and the end of its passes; 0.01 us units), against
        # the launch's earliest entry
        na = int(alive.sum())
        rows = np.concatenate([s2[:N][alive], s2[N:][alive]]) if split else s2[:N][alive]
        is_obs = np.concatenate([np.zeros(na, bool), np.ones(na, bool)]) if split else np.zeros(na, bool)
        t0 = int(rows[0, 9]) + int(rel(rows[:, 9], rows[0, 9]).min())
        ent, end = rel(rows[:, 9], t0) / 100.0, rel(rows[:, 10], t0) / 100.0
        ped_end = end[~is_obs]
        print(f'  us since the launch\'s earliest entry: pedestrian passes end median {np.median(ped_end):6.2f}  p90 {np.percentile(ped_end, 90):6.2f}  last {ped_end.max():6.2f}')
        if split:
            print(f'    obstacle workgroups\' waves enter first {ent[is_obs].min():6.2f}  median {np.median(ent[is_obs]):6.2f}  last {ent[is_obs].max():6.2f};'
                  f'  their passes end median {np.median(end[is_obs]):6.2f}  last {end[is_obs].max():6.2f}')
            print(f'    pedestrian workgroups\' waves enter first {ent[~is_obs].min():6.2f}  median {np.median(ent[~is_obs]):6.2f}  last {ent[~is_obs].max():6.2f}')
        b = pk[pk[:, 1] != 0]
        if len(b):
            st_, en_ = rel(b[:, 0], t0) / 100.0, rel(b[:, 1], t0) / 100.0
            print(f'  {len(b)} pack blocks: first start {st_.min():6.2f}  median start {np.median(st_):6.2f}  last start {st_.max():6.2f}  last end {en_.max():6.2f} us;'
                  f'  median length {np.median(b[:, 2]):6.0f} ticks = {np.median(en_ - st_):5.2f} us')
            print(f'    last pack end - last pedestrian pass end: {en_.max() - ped_end.max():+6.2f} us;  pack blocks still running at the last pedestrian pass end: {int((en_ > ped_end.max()).sum())};'
                  f'  starting behind it: {int((st_ > ped_end.max()).sum())}')
if hasattr(L, 'piml_relfeat_pack_form'):
    L.piml_relfeat_pack_form(0)
