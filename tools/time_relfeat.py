"""Device timing of the relfeat kernels, launched back to back through the C ABI so the GPU
(not the Python host) is the bottleneck (development aid)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from piml_amd import ops, _lib
from piml_amd.scenes import synthetic_gc_scene, pair_count, algorithmic_bytes

L = _lib.lib()
dev = 'cuda:0'


def time_with_pack():
    """--pack: the forward launch of a step WITH the step's deferred weight pack in it (PIML_DEFER_PACK), per form of
    piml_relfeat_pack_form (0 = trailing workgroups, the default; 1 = the obstacle workgroups' tail), next to the launch
    without a pack: R launches captured into one graph, so the device and not the host sets the pace.  A library without the switch
    (an older build of the same tree layout) prints its only form."""
    import types
    import piml_amd.models.model as MODEL
    args = types.SimpleNamespace(
        ped_feature_dim=6, obs_feature_dim=6, self_feature_dim=7, encoder_hidden_size=128, processor_hidden_size=128,
        decoder_hidden_size=64, encoder_hidden_layers=3, processor_hidden_layers=16, decoder_hidden_layers=2, dropout=0.5,
        activation='relu', dataset_name='ucy', res_hidden_layers=3, correction_hidden_layers=1, time_unit=0.08, collision_threshold=0.5)
    torch.manual_seed(0)
    model = MODEL.PINNSF_multitask(args).to(dev).eval()
    model.messages_wanted = False                       # the benchmarked step: plain images + the folded ones
    spec, fold = model._pack_spec(), model._fold_spec()
    packs = ops.PinnsfPacks()
    forms = (0, 1) if hasattr(L, 'piml_relfeat_pack_form') else (None,)
    R, K = 20, 25
    import numpy as np
    for N, M, FC in ((122, 2000, None), (488, 2000, None), (1024, 2000, None), (4096, 2000, None), (16384, 2000, 2048)):
        sc = synthetic_gc_scene(N, M, seed=0)
        state = torch.tensor(np.concatenate([sc['position'], sc['velocity'], sc['acceleration']], axis=-1), device=dev)
        dest, obs, v0 = (torch.tensor(sc[k], device=dev) for k in ('destination', 'obstacles', 'desired_speed'))
        fc = FC or N
        dest, v0 = dest[:fc].contiguous(), v0[:fc].contiguous()
        line = f'N_focal={fc} N_src={N} M={obs.shape[0]}:'
        for form in ('none',) + forms:
            if form not in ('none', None):
                L.piml_relfeat_pack_form(form)

            def body():
                with torch.no_grad():
                    for _ in range(R):
                        if form != 'none':
                            ops.pinnsf_prepack(packs, *spec, defer=True, fold=fold)
                        ops.relative_features_packed_self(state, dest, obs, v0, 0, fc)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            samples = []
            for _ in range(5):
                g.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K):
                    g.replay()
                e1.record(); torch.cuda.synchronize()
                samples.append(e0.elapsed_time(e1) * 1e3 / (K * R))
            name = {'none': 'no pack', None: 'with pack', 0: 'trailing', 1: 'tail'}[form]
            line += f'  {name} {np.median(samples):.2f} ({min(samples):.2f} - {max(samples):.2f})'
        print(line + ' us', flush=True)
    if forms != (None,):
        L.piml_relfeat_pack_form(0)


if '--pack' in sys.argv:
    time_with_pack()
    sys.exit(0)
# (N, M, C, focal rows): the last entry is the launch every rank of the 8-GPU run executes (cfg4: 2048 focal rows against 16384 sources)
for N, M, C, FC in ((122, 100, 1, None), (1024, 100, 1, None), (4096, 2000, 1, None), (16384, 2000, 1, None), (128, 100, 64, None), (16384, 2000, 1, 2048)):
    sc = synthetic_gc_scene(N, M, seed=0, channels=None if C == 1 else C)
    p, v, a, d, o = [torch.tensor(sc[k], device=dev) for k in ('position', 'velocity', 'acceleration', 'destination', 'obstacles')]
    pf, of, df, pi, oi = ops.relative_features(p, v, a, d, o, return_index=True)
    st = torch.cuda.current_stream().cuda_stream
    cp, co = ops.cos_threshold(90), ops.cos_threshold(90)
    Me = o.shape[0]

    fc = FC or N

    def fwd():
        return L.piml_relfeat_fwd(p.data_ptr(), None, v.data_ptr(), a.data_ptr(), 2, d.data_ptr(), o.data_ptr(), C, N, Me, 0, fc,
                                  6, 10, cp, co, 4.0, 4.0, pf.data_ptr(), of.data_ptr(), df.data_ptr(), 2, pi.data_ptr(), oi.data_ptr(), st)
    gs = torch.zeros(*p.shape[:-1], 6, device=dev); gd = torch.empty_like(df)
    gp, go = torch.randn_like(pf), torch.randn_like(of)

    def bwd():
        return L.piml_relfeat_bwd(gp.data_ptr(), go.data_ptr(), df.data_ptr(), pi.data_ptr(), oi.data_ptr(), p.data_ptr(), 2, d.data_ptr(),
                                  C, N, 0, N, pf.shape[-2], of.shape[-2], gs.data_ptr(), gd.data_ptr(), st)
    for name, fn in ((('fwd', fwd), ('bwd', bwd)) if FC is None else (('fwd', fwd),)):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 300
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        pairs = C * pair_count(N, Me) * fc // N
        extra = f'{pairs / us * 1e6:.3e} pairs/s, alg {C * algorithmic_bytes(N, Me) / us / 1e3:.0f} GB/s' if name == 'fwd' else ''
        print(f'C={C} N_focal={fc} N_src={N} M={Me} {name}: {us:.2f} us  {extra}')
