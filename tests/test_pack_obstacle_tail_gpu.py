"""GPU: the two places a deferred weight pack (PIML_DEFER_PACK, piml_amd/csrc/reduce.hpp: PackWork) can ride in the relative-feature
forward launch -- as trailing workgroups, or in the tail of a split launch's obstacle workgroups (piml_relfeat_pack_form) -- against the
pack as a launch of its own.  The pack blocks, their thread count and their arithmetic are the same in all three, and the search does
not read what the pack writes, so everything is compared BITWISE (as bit patterns: NaN scenes included):

  * the operand images of every encoder branch, decoder branch and the head, with 256-byte guard bands around each buffer;
  * the relative features and both index tensors, with the launch that carries no pack;
  * the model's acceleration and every weight gradient.

The buffers are refilled with a sentinel and the weights rescaled before every pass, so a pack that did not run, ran on stale weights
or left an element out shows.  Reference: the step of src/models/simulators.py:699-779 (features, network, backward), whose weights
the reference reads in place -- the images are this port's derived data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64                      # floats: 256 bytes either side of every packed buffer
SENTINEL = -12345.5
FORMS = ('standalone', 0, 1)    # the pack as its own launch | trailing workgroups | the obstacle workgroups' tail


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _scene(N, M, seed=3, absent=False, far=False, channels=None):
    from piml_amd.scenes import synthetic_gc_scene
    sc = synthetic_gc_scene(N, M, seed=seed, channels=channels)
    state = torch.tensor(np.concatenate([sc['position'], sc['velocity'], sc['acceleration']], axis=-1), device=DEV)
    if absent:
        state[:] = float('nan')
    obs = torch.tensor(sc['obstacles'], device=DEV)[:M]
    if far:
        obs = obs + 1000.0      # the hall is tens of metres wide: nobody is within the 4 m range
    return state, torch.tensor(sc['destination'], device=DEV), obs, torch.tensor(sc['desired_speed'], device=DEV)


def _model(cls='PINNSF_multitask', train=False, messages=True):
    import piml_amd.models.model as MODEL
    from piml_amd import ops, _lib
    from test_mlpglue_gpu import model_args
    torch.manual_seed(5)
    m = getattr(MODEL, cls)(model_args()).to(DEV)
    m = m.train() if train else m.eval()
    m.messages_wanted = messages
    # guarded operand-image buffers: the model packs into views whose rows have GUARD floats of sentinel either side
    L = _lib.lib()
    m._packs = ops.PinnsfPacks()
    sizes = (L.piml_encoder_pack_floats(), L.piml_decoder_pack_floats(), L.piml_collision_head_pack_floats())
    m._guarded = [torch.empty(2, sizes[0] + 2 * GUARD, device=DEV), torch.empty(2, sizes[1] + 2 * GUARD, device=DEV),
                  torch.empty(1, sizes[2] + 2 * GUARD, device=DEV)]
    m._packs.epack = m._guarded[0][:, GUARD:GUARD + sizes[0]]
    m._packs.dpack = m._guarded[1][:, GUARD:GUARD + sizes[1]]
    m._packs.hpack = m._guarded[2][0, GUARD:GUARD + sizes[2]]
    m._base = [p.detach().clone() for p in m.parameters()]
    return m


def _one_pass(model, scene, form, factor, monkeypatch, features='packed_self', run_model=True, relfeat_inside=True, feats_outside=None):
    """one step under `form`: returns the guarded image buffers, the features + indices, the acceleration and the weight gradients"""
    from piml_amd import ops, _lib
    state, dest, obs, v0 = scene
    with torch.no_grad():
        for p, b in zip(model.parameters(), model._base):
            p.copy_(b * factor)
            p.grad = None
    for g in model._guarded:
        g.fill_(SENTINEL)
    monkeypatch.setattr(ops, 'DEFER_PACK', form != 'standalone')
    if form != 'standalone':
        _lib.lib().piml_relfeat_pack_form(form)
    ops.dropout_seed(11)                                # the same dropout draws in every pass (seed, call counter back to 0)
    out = {}
    with model.packed_weights():
        if not relfeat_inside:
            feats = feats_outside
        elif features == 'packed_self':
            N = state.shape[0]
            feats = ops.relative_features_packed_self(state, dest, obs, v0, 0, N, return_index=True)
        elif features == 'local_remote':                # the pack rides in the LOCAL part
            N = state.shape[0]
            f0, fc = N // 4, N // 2
            d_rows, v_rows = dest[f0:f0 + fc].contiguous(), v0[f0:f0 + fc].contiguous()
            loc = ops.relative_features_local_part(state, d_rows, obs, v_rows, f0, fc)
            feats = ops.relative_features_packed_self(state, d_rows, obs, v_rows, f0, fc, return_index=True, local=loc)
        elif features == 'separate':                    # (..., N, 2) inputs, any number of slices; topk_obs as given
            feats = ops.relative_features(state[..., 0:2].contiguous(), state[..., 2:4].contiguous(), state[..., 4:6].contiguous(),
                                          dest, obs, return_index=True)
        elif features == 'no_obstacle_slots':
            feats = ops.relative_features(state[..., 0:2].contiguous(), state[..., 2:4].contiguous(), state[..., 4:6].contiguous(),
                                          dest, obs, topk_obs=0, return_index=True)
        if relfeat_inside:
            torch.cuda.synchronize()
            out['images_behind_relfeat'] = [g.clone() for g in model._guarded]     # the pack has run by now in every form
        if run_model:
            acc = model(*feats[:3])[0]
            acc.backward(torch.ones_like(acc))
            out['acc'] = acc.detach().clone()
            out['grads'] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    torch.cuda.synchronize()
    out['images'] = [g.clone() for g in model._guarded]
    out['feats'] = [f.detach().clone() for f in feats]
    return out


def _check_guards(model, images):
    for g in images:
        assert bool((g[:, :GUARD] == SENTINEL).all()) and bool((g[:, -GUARD:] == SENTINEL).all()), 'a guard band was written'
    assert bool((images[0][:, GUARD:-GUARD] != SENTINEL).any()), 'no encoder image was written'


def _compare(model, want, got, what):
    for key in want:
        a, b = want[key], got[key]
        if torch.is_tensor(a):
            a, b = [a], [b]
        assert len(a) == len(b), (what, key)
        for i, (x, y) in enumerate(zip(a, b)):
            assert _same(x, y), f'{what}: {key}[{i}] differs'
    _check_guards(model, got['images'])


def _run_forms(model, scene, monkeypatch, forms=FORMS, factors=(1.0, 1.25), **kw):
    from piml_amd import _lib
    old = _lib.lib().piml_relfeat_pack_form(-1)
    try:
        for factor in factors:
            want = _one_pass(model, scene, forms[0], factor, monkeypatch, **kw)
            _check_guards(model, want['images'])
            if 'grads' in want:
                assert len(want['grads']) > 10
            for form in forms[1:]:
                _compare(model, want, _one_pass(model, scene, form, factor, monkeypatch, **kw), (form, factor))
    finally:
        _lib.lib().piml_relfeat_pack_form(old)


# N, M, PIML_RELFEAT_WAVES (None = the launch's own choice), scene options.  Obstacle workgroups = ceil(N / waves).
SHAPES = {
    'n5_w4_two_workgroups_three_idle_waves': (5, 300, 4, {}),        # the second workgroup: one live row, three waves without
    'n40_w16_last_has_8_rows': (40, 300, 16, {}),
    'n122_natural': (122, 300, None, {}),                            # four waves, 31 obstacle workgroups of 28 blocks each
    'n1024_natural': (1024, 300, None, {}),                          # eight waves, 128 obstacle workgroups of 6
    'n4096_natural': (4096, 300, None, {}),                          # sixteen waves alone, eight with a pack on board: the same bits
    'all_agents_absent': (40, 300, 4, dict(absent=True)),
    'nobody_in_range_of_an_obstacle': (40, 300, 4, dict(far=True)),
    'm2049_past_the_resident_tile': (40, 2049, 4, {}),
}


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_both_forms_are_bitwise_the_standalone_pack(shape, monkeypatch):
    N, M, waves, opt = SHAPES[shape]
    if waves is None:
        monkeypatch.delenv('PIML_RELFEAT_WAVES', raising=False)
    else:
        monkeypatch.setenv('PIML_RELFEAT_WAVES', str(waves))
    model, scene = _model(), _scene(N, M, **opt)
    assert scene[2].shape[0] == M
    _run_forms(model, scene, monkeypatch)


@pytest.mark.parametrize('case', ['no_obstacles', 'no_obstacle_slots', 'two_slices_of_64', 'two_slices_not_split'])
def test_launches_without_obstacle_workgroups_keep_the_trailing_form(case, monkeypatch):
    """M = 0 or topk_obs = 0: no obstacle pass exists; C = 2 slices above 4096 rows: the launch is not split.  Forcing the tail form must
    leave such a launch on the trailing one -- the pack still runs (two slices of 64 agents: whichever form the launch takes)."""
    monkeypatch.setenv('PIML_RELFEAT_WAVES', '4')
    model = _model()
    if case == 'no_obstacles':
        scene = _scene(40, 0)
        assert scene[2].shape[0] == 0
        kw = dict(features='separate')
    elif case == 'no_obstacle_slots':
        scene, kw = _scene(40, 300), dict(features='no_obstacle_slots')
    elif case == 'two_slices_of_64':
        scene, kw = _scene(64, 300, channels=2), dict(features='separate')
    else:
        monkeypatch.setenv('PIML_RELFEAT_WAVES', '16')
        scene, kw = _scene(2100, 300, channels=2), dict(features='separate')      # 4200 rows > 4096, C > 1
    _run_forms(model, scene, monkeypatch, factors=(1.0,), run_model=False, **kw)


def test_pack_rides_in_the_local_part_of_a_sharded_launch(monkeypatch):
    monkeypatch.setenv('PIML_RELFEAT_WAVES', '4')
    _run_forms(_model(), _scene(80, 300), monkeypatch, features='local_remote')


@pytest.mark.parametrize('case', ['train_mode_dropout', 'sums_path_with_fold', 'pinnsf_bm'])
def test_other_image_sets(case, monkeypatch):
    """train mode with dropout and messages_wanted: no folded images; messages not wanted (the benchmarked step): the fold blocks and the
    head's; pinnsf_bm: neither fold nor head.  All with the f32 fragment images skipped (the default products)."""
    monkeypatch.setenv('PIML_RELFEAT_WAVES', '4')
    if case == 'train_mode_dropout':
        model = _model(train=True, messages=True)
    elif case == 'sums_path_with_fold':
        model = _model(messages=False)
    else:
        model = _model('PINNSF_bottleneck_multitask')
    _run_forms(model, _scene(40, 300), monkeypatch)


def test_block_without_a_relfeat_launch_flushes_as_before(monkeypatch):
    from piml_amd import ops
    model, scene = _model(), _scene(40, 300)
    feats = ops.relative_features_packed_self(*scene, 0, 40, return_index=True)
    _run_forms(model, scene, monkeypatch, relfeat_inside=False, feats_outside=feats)


@pytest.mark.parametrize('form', [0, 1])
def test_captured_step_replays_bitwise(form, monkeypatch):
    import piml_amd
    from piml_amd import ops, _lib
    if not piml_amd.hip_graphs_safe():
        pytest.skip('HIP graphs not trusted in this process')
    monkeypatch.setenv('PIML_RELFEAT_WAVES', '4')
    model, scene = _model(), _scene(40, 300)
    state, dest, obs, v0 = scene
    want = _one_pass(model, scene, 'standalone', 1.0, monkeypatch)
    old = _lib.lib().piml_relfeat_pack_form(form)
    monkeypatch.setattr(ops, 'DEFER_PACK', True)
    keep = {}

    def body():
        for p in model.parameters():
            p.grad = None
        with model.packed_weights():
            keep['feats'] = ops.relative_features_packed_self(state, dest, obs, v0, 0, 40, return_index=True)
            keep['acc'] = model(*keep['feats'][:3])[0]
            keep['acc'].backward(torch.ones_like(keep['acc']))
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        for replay in range(3):
            for buf in model._guarded:
                buf.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            got = dict(images=[b.clone() for b in model._guarded], feats=list(keep['feats']), acc=keep['acc'].detach(),
                       grads=[p.grad for p in model.parameters() if p.grad is not None])
            _compare(model, {k: want[k] for k in got}, got, ('replay', replay))
    finally:
        _lib.lib().piml_relfeat_pack_form(old)
