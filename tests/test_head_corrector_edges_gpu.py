"""GPU: the corrector of `pinnsf_res` (ops.fused_corrector, piml_amd/csrc/corrector.hip) and the collision head of `pinnsf_bm`
(ops.collision_head64, piml_amd/csrc/head64.hip) against float64 past the shapes of their first tests
(test_corrector_gpu.py, test_encoder_gpu.py::test_collision_head64_matches_float64):

  corrector  a second and a third pass of the per-agent kernels' grid loop (more than 4096 agents), k = 1 / 64 / between 32 and
             64, 128 and 129 agents and rows (the slot boundaries of both weight-gradient workgroup kinds, a rows workgroup with
             empty tiles), an input without gradient, weights without gradient, accumulation under a ParamGradSink, refusals
  head64     the last one-tile-per-workgroup size (65536 rows) and the first four-tile one (65537), a ragged last tile and
             empty waves in the last workgroup, an input without gradient, a dead hidden layer, a saturated sigmoid,
             piml_head64_bwd_acc(accumulate = 1) called directly

Bar: max |got - ref| / max |ref| <= 1e-5 per tensor (the north-star bar of the first tests), the measured value printed.  The
float64 references are those of the first tests.  Inputs are re-drawn, in float64 on the reference alone, until no ReLU
pre-activation lies within 1e-5 of its layer's mean magnitude of zero (test_encoder_gpu.dodge_relu_kinks says why): a test
begins only when NO row is left inside that margin."""
import ctypes

import pytest
import torch

from test_corrector_gpu import _modules, _reference

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINK = 1e-5
CORR_NAMES = ['enc', 'wa', 'ba', 'wb', 'bb', 'wc', 'bc', 'wd', 'bd']


# ---------------------------------------------------------------------------------------------------------------- corrector

def _params(pool, tail):
    gw, tl = pool.get_weights.mlp, tail.mlp
    return [gw[0].weight, gw[0].bias, gw[2].weight, gw[2].bias, tl[0].weight, tl[0].bias, tl[2].weight, tl[2].bias]


def _corrector_near_kink(enc, scale, keep, params):
    """(..., N) bool: the agents with a pre-activation of `Wa r + ba` (any of their k rows) or of `Wc pooled + bc` within
    KINK x the layer's mean magnitude of zero, in float64."""
    w = [p.detach().double() for p in params]
    r = enc.detach().double() * scale
    if keep is not None:
        r = r * keep.double()
    za = r @ w[0].t() + w[1]
    s = torch.relu(za) @ w[2].t() + w[3]
    pooled = (r * torch.softmax(torch.exp(s), dim=-2)).sum(-2)
    zc = pooled @ w[4].t() + w[5]
    return (za.abs() < KINK * za.abs().mean()).any(-1).any(-1) | (zc.abs() < KINK * zc.abs().mean()).any(-1)


def _corrector_dodge(enc, scale, keep, params, rounds=12):
    """Re-draw every row of the agents near a kink (`pooled` depends on all k of them)."""
    g = torch.Generator().manual_seed(4321)
    with torch.no_grad():
        for _ in range(rounds):
            bad = _corrector_near_kink(enc, scale, keep, params)
            n = int(bad.sum())
            if n == 0:
                return enc
            enc[bad] = (torch.randn(n, *enc.shape[-2:], generator=g) * 0.5).to(DEV)
    raise AssertionError('_corrector_dodge: still near a kink after re-drawing')


def _corrector_case(shape, train, seed=7, dodge=True):
    from piml_amd import ops
    res, pool, tail = _modules()
    params = _params(pool, tail)
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(*shape, 128, generator=g) * 0.5).to(DEV)
    gout = torch.randn(*shape[:-1], 2, generator=g).to(DEV)
    rows = enc.numel() // 128
    keep, bits, scale = None, None, 2.0
    if train:
        keep = (torch.rand(rows, 128, generator=g) < 0.5).to(DEV)
        bits = ops.pack_keep_bits(keep)
        keep = keep.view(*shape, 128)
        scale = 4.0
    if dodge:
        _corrector_dodge(enc, scale, keep, params)
        assert int(_corrector_near_kink(enc, scale, keep, params).sum()) == 0
    return dict(enc=enc.requires_grad_(True), gout=gout, keep=keep, bits=bits, scale=scale, params=params, pool=pool, tail=tail)


def _corrector_run(c, enc_grad=True, weight_grad=True):
    """[out, g_enc (if asked), the eight weight gradients (if asked)] of one forward and backward pass."""
    from piml_amd import ops
    enc = c['enc'] if enc_grad else c['enc'].detach()
    ps = c['params'] if weight_grad else [p.detach() for p in c['params']]
    out = ops.fused_corrector(enc, c['scale'], c['bits'], ps[:4], ps[4:])
    leaves = ([enc] if enc_grad else []) + (list(ps) if weight_grad else [])
    return [out.detach()] + list(torch.autograd.grad(out, leaves, c['gout']))


def _rel(a, b, scale=None):
    a, b = a.detach().double(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() if scale is None else scale).clamp_min(1e-30))


def _corrector_forward_buffers(c):
    """piml_corrector_fwd called as _Corrector.forward calls it -> (attn, pooled, out)."""
    from piml_amd import _lib, ops
    enc, k = c['enc'].detach(), c['enc'].shape[-2]
    rows = enc.numel() // 128
    agents = rows // k
    opt = dict(device=enc.device, dtype=torch.float32)
    score, attn = torch.empty(rows, **opt), torch.empty(rows, **opt)
    pooled, chid, out = torch.empty(agents, 128, **opt), torch.empty(agents, 64, **opt), torch.empty(agents, 2, **opt)
    wb = [p.detach().contiguous() for p in c['params']]
    C = _lib.Corrector()
    C.agents, C.k, C.scale = agents, k, float(c['scale'])
    C.enc, C.keep_bits = enc.data_ptr(), ops._ptr(c['bits'])
    C.wa, C.ba, C.wb, C.bb, C.wc, C.bc, C.wd, C.bd = [t.data_ptr() for t in wb]
    C.score, C.attn, C.pooled, C.chid, C.out = score.data_ptr(), attn.data_ptr(), pooled.data_ptr(), chid.data_ptr(), out.data_ptr()
    _lib.check(_lib.lib().piml_corrector_fwd(ctypes.byref(C), ops._stream()), 'piml_corrector_fwd')
    torch.cuda.synchronize()
    return attn, pooled, out


CORR_SHAPES = [(4097, 1),           # a second pass of the agents' grid loop with one agent in it; k = 1
               (8197, 2),           # a third pass; agents no multiple of 4
               (128, 1), (129, 1),  # one -> two slots of both partial sets at once; a rows workgroup with three empty tiles
               (43, 3),             # 129 rows from a k that does not divide 32
               (5, 64),             # the largest k: every lane live
               (7, 33),             # an agent's rows span two 32-row tiles
               (2, 5, 33)]          # the same under a leading dimension
CORR_CASES = [(s, False) for s in CORR_SHAPES] + [((4097, 1), True), ((129, 1), True), ((7, 33), True)]


@pytest.mark.parametrize('shape,train', CORR_CASES)
def test_fused_corrector_edges_match_float64(shape, train):
    """Output and all nine gradients against float64, eval mode and train mode (injected keep mask, scale 4).  The `bb` rule is
    test_fused_corrector_matches_float64's: its gradient is a sum of score gradients that cancel per agent, so its error is
    measured against the size of the terms (the `wb` gradient's).

    k = 1 in addition: the softmax over one row is exactly 1 -- `attn` == 1 and `pooled` == keep * scale * enc bit for bit, read
    from piml_corrector_fwd's own buffers (two float32 evaluations of the tail's dot products agree to rounding only, so `out`
    itself is held against the float32 tail of that r at the bar, not bitwise) -- and the score gradient exactly 0, visible as
    the gradients of wa, ba, wb, bb being exactly zero (as they are in float64).

    Measured on an MI355X, worst of out and the nine gradients per case: (4097, 1) 2.2e-7, train 2.5e-7; (8197, 2) 5.1e-7;
    (128, 1) 3.0e-7; (129, 1) 2.7e-7, train 2.7e-7; (43, 3) 4.1e-7; (5, 64) 5.7e-7; (7, 33) 6.9e-7, train 4.3e-7;
    (2, 5, 33) 4.3e-7 (a record, not a bar)."""
    c = _corrector_case(shape, train)
    got = _corrector_run(c)
    want, wgrads = _reference(c['enc'], c['scale'], c['keep'], c['pool'], c['tail'], c['gout'])
    torch.cuda.synchronize()
    out, grads = got[0], got[1:]
    assert out.shape == want.shape == (*shape[:-1], 2)
    worst = {'out': _rel(out, want)}
    for name, a, b in zip(CORR_NAMES, grads, wgrads):
        assert a.shape == b.shape, name
        assert torch.isfinite(a).all(), name
        worst['g_' + name] = _rel(a, b, scale=torch.maximum(wgrads[3].abs().max(), b.abs().max()) if name == 'bb' else None)
    print(shape, 'train' if train else 'eval', {k: f'{v:.1e}' for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1e-5, (name, v)
    if shape[-1] == 1:
        attn, pooled, out2 = _corrector_forward_buffers(c)
        r32 = c['enc'].detach() * c['scale']
        if c['keep'] is not None:
            r32 = torch.where(c['keep'], r32, torch.zeros_like(r32))
        assert torch.equal(attn, torch.ones_like(attn))
        assert torch.equal(pooled, r32.reshape(-1, 128))
        assert torch.equal(out2.view_as(out), out)
        wc, bc, wd, bd = [p.detach() for p in c['params'][4:]]
        tail32 = (torch.relu(r32.reshape(-1, 128) @ wc.t() + bc) @ wd.t() + bd).view_as(out)
        assert _rel(out, tail32.double()) <= 1e-5
        for name, a, b in list(zip(CORR_NAMES, grads, wgrads))[1:5]:
            assert not b.any(), name                    # float64: softmax of one element is 1, its backward g - g
            assert not a.any(), name


@pytest.fixture(scope='module')
def corr3():
    """(4097, 3): the case and its full run (out, g_enc, eight weight gradients), shared by the tests below and left unchanged."""
    c = _corrector_case((4097, 3), False, seed=13, dodge=False)
    return c, _corrector_run(c)


def test_fused_corrector_second_pass_is_bit_reproducible(corr3):
    c, full = corr3
    again = _corrector_run(c)
    assert len(again) == len(full) == 10
    for name, a, b in zip(['out'] + CORR_NAMES, full, again):
        assert torch.equal(a, b), name


def test_fused_corrector_input_without_gradient(corr3):
    """A.g_enc == nullptr: the rows kernel skips g_r and the `enc` gradient's stores; the weight gradients are the same sums."""
    c, full = corr3
    got = _corrector_run(c, enc_grad=False)
    assert len(got) == 9 and torch.equal(got[0], full[0])
    for name, a, b in zip(CORR_NAMES[1:], got[1:], full[2:]):
        assert torch.equal(a, b), name


def test_fused_corrector_weights_without_gradient(corr3):
    c, full = corr3
    got = _corrector_run(c, weight_grad=False)
    assert len(got) == 2 and torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])


def test_fused_corrector_under_a_param_grad_sink(corr3):
    """Two backward passes inside one ParamGradSink step (the usage of test_param_grad_sink_equals_autograd_accumulation): the
    second pass's slot sums add into the first's (piml_corrector_bwd, accumulate = 1).  sum_slots_16x16_at (pack.hpp) finishes the
    slot sum in registers and then adds the old value to it once (slot_sum_store: s += *dst; *dst = s), so the result is ONE
    float32 addition of the two passes' stand-alone gradients, whichever pass runs first: asserted bitwise."""
    from piml_amd import ops
    c1, full1 = corr3
    c2 = _corrector_case((4097, 3), False, seed=29, dodge=False)
    full2 = _corrector_run(c2)
    params = c1['params']
    for p, q in zip(params, c2['params']):
        with torch.no_grad():
            assert torch.equal(p, q)                    # (_modules() is seeded: the same weights)
    encs = [c['enc'].detach().clone().requires_grad_(True) for c in (c1, c2)]
    for p in params:
        p.grad = None
    sink = ops.ParamGradSink()
    with sink.step():
        loss = 0
        for e, c in zip(encs, (c1, c2)):
            out = ops.fused_corrector(e, c['scale'], None, params[:4], params[4:])
            loss = loss + (out * c['gout']).sum()
        loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(encs[0].grad, full1[1]) and torch.equal(encs[1].grad, full2[1])
    for name, p, a, b in zip(CORR_NAMES[1:], params, full1[2:], full2[2:]):
        assert p.grad is not None, name
        assert torch.equal(p.grad, a + b), name
        assert bool((p.grad != a).any()) or not bool(b.any()), name      # (it did accumulate)
    for p in params:
        p.grad = None


def test_fused_corrector_refusals():
    from piml_amd import ops
    res, pool, tail = _modules()
    p = [t.detach() for t in _params(pool, tail)]
    enc = torch.zeros(3, 6, 128, device=DEV)
    with pytest.raises(ValueError):
        ops.fused_corrector(torch.zeros(3, 65, 128, device=DEV), 2.0, None, p[:4], p[4:])            # k = 65
    with pytest.raises(ValueError):
        ops.fused_corrector(torch.zeros(18, 128, device=DEV), 2.0, None, p[:4], p[4:])               # no k axis
    with pytest.raises(ValueError):
        ops.fused_corrector(enc, 2.0, None, p[:4], [torch.zeros(64, 64, device=DEV)] + p[5:])        # wc (64, 64)
    with pytest.raises(ValueError):
        ops.fused_corrector(enc, 4.0, torch.zeros(18, 4, dtype=torch.int64, device=DEV), p[:4], p[4:])
    with pytest.raises(ValueError):
        ops.fused_corrector(enc, 4.0, torch.zeros(18, 3, dtype=torch.int32, device=DEV), p[:4], p[4:])
    out = ops.fused_corrector(enc, 4.0, torch.zeros(18, 4, dtype=torch.int32, device=DEV), p[:4], p[4:])   # (the accepted form)
    assert out.shape == (3, 2)


# ------------------------------------------------------------------------------------------------------------------- head64

HEAD_NAMES = ['out', 'g_x', 'dW1', 'db1', 'dw2', 'db2']
HEAD_SIZES = [65537, 97]            # four tiles per workgroup (head64_bwd_kernel) | one (head64_bwd_coop_kernel)


def _head_near_kink(x, w):
    z = x.detach().double() @ w[0].detach().double().t() + w[1].detach().double()
    return (z.abs() < KINK * z.abs().mean()).any(-1)


def _head_case(rows, b1=None, b2=None, w2_scale=1.0, rounds=12):
    """x, the four weights and the upstream gradient as test_collision_head64_matches_float64 draws them; rows of x re-drawn
    until no pre-activation of `W1 x + b1` is near zero."""
    rows = rows if isinstance(rows, tuple) else (rows,)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(*rows, 64, generator=g).to(DEV)
    w = [(torch.randn(*d, generator=g) * (0.3 if len(d) == 2 else 0.1)).to(DEV) for d in [(64, 64), (64,), (1, 64), (1,)]]
    go = torch.randn(*rows, generator=g).to(DEV)
    if b1 is not None:
        w[1].fill_(b1)
    if b2 is not None:
        w[3].fill_(b2)
    w[2].mul_(w2_scale)
    for _ in range(rounds):
        bad = _head_near_kink(x, w)
        n = int(bad.sum())
        if n == 0:
            break
        x[bad] = torch.randn(n, 64, generator=g).to(DEV)
    assert int(_head_near_kink(x, w).sum()) == 0
    return x.requires_grad_(True), [t.requires_grad_(True) for t in w], go


def _head_run(x, w, go, x_grad=True):
    from piml_amd import ops
    xx = x if x_grad else x.detach()
    out = ops.collision_head64(xx, *w)
    return [out.detach().clone()] + [t.clone() for t in torch.autograd.grad((out * go).sum(), ([xx] if x_grad else []) + list(w))]


def _head_reference(x, w, go, b2=None):
    xd = x.detach().double().requires_grad_(True)
    wd = [t.detach().double().requires_grad_(True) for t in w]
    if b2 is not None:
        wd[3] = torch.full_like(wd[3], b2).requires_grad_(True)
    ref = torch.sigmoid(torch.relu(xd @ wd[0].t() + wd[1]) @ wd[2].t() + wd[3]).squeeze(-1)
    return [ref.detach()] + list(torch.autograd.grad((ref * go.double()).sum(), [xd, *wd]))


@pytest.mark.parametrize('rows', [65536,                # the last one-tile-per-workgroup size: 2048 tiles, 2048 slots
                                  65537,                # the first four-tile size: the last workgroup has one row, three empty waves
                                  65536 + 128 + 33,     # last workgroup: a full tile, a ragged tile, two empty waves
                                  (3, 21846)])          # a leading dimension across the bound
def test_collision_head64_edges_match_float64(rows):
    """Output and all five gradients against float64 at the dispatch bound between the two backward kernels and with a ragged
    last workgroup of the four-tile one; run twice, bit for bit the same.  Bar and normalisation of
    test_collision_head64_matches_float64.  Measured on an MI355X (worst of the six tensors): 65536 rows 8.9e-7, 65537 7.7e-7,
    65697 5.7e-7, (3, 21846) 7.5e-7 (a record, not a bar)."""
    x, w, go = _head_case(rows)
    runs = [_head_run(x, w, go) for _ in range(2)]
    for name, a, b in zip(HEAD_NAMES, *runs):
        assert torch.equal(a, b), name
    worst = {}
    for name, a, b in zip(HEAD_NAMES, runs[0], _head_reference(x, w, go)):
        assert a.shape == b.shape, name
        worst[name] = _rel(a, b)
    print(f'collision_head64 rows={rows}:', {k: f'{v:.1e}' for k, v in worst.items()})
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.parametrize('rows', HEAD_SIZES)
def test_collision_head64_input_without_gradient(rows):
    """A.g_x == nullptr in both backward kernels: the weight gradients are the same sums."""
    x, w, go = _head_case(rows)
    full, part = _head_run(x, w, go), _head_run(x, w, go, x_grad=False)
    assert len(part) == 5 and torch.equal(part[0], full[0])
    for name, a, b in zip(HEAD_NAMES[2:], part[1:], full[2:]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize('rows', HEAD_SIZES)
def test_collision_head64_dead_hidden_layer(rows):
    """b1 = -1e3: no hidden unit fires (the `hh > 0` predicate false everywhere).  out = sigmoid(b2) on every row, g_x, dW1, db1
    and dw2 exactly zero -- in the kernels and in float64 -- and db2 under the bar."""
    x, w, go = _head_case(rows, b1=-1e3)
    got, ref = _head_run(x, w, go), _head_reference(x, w, go)
    assert torch.equal(ref[0], torch.sigmoid(w[3].detach().double()).expand_as(ref[0]))
    assert torch.equal(got[0], got[0].flatten()[0].expand_as(got[0]))
    assert _rel(got[0], ref[0]) <= 1e-5
    for name, a, b in list(zip(HEAD_NAMES, got, ref))[1:5]:
        assert not b.any(), name
        assert not a.any(), name
    err = _rel(got[5], ref[5])
    print(f'collision_head64 dead hidden layer rows={rows}: db2 {err:.1e}')
    assert err <= 1e-5


@pytest.mark.parametrize('b2', [40.0, -40.0, -120.0])
@pytest.mark.parametrize('rows', HEAD_SIZES)
def test_collision_head64_saturated_sigmoid(rows, b2):
    """A saturated output (w2 at a tenth of its usual scale, so that b2 decides every row alike).
      b2 = +40   float32 1 / (1 + exp(-40)) is exactly 1: every output 1, gz = g o (1 - o) exactly 0, every gradient exactly 0
      b2 = -120  exp(120) overflows float32, 1 / inf: every output exactly 0, every gradient exactly 0
      b2 = -40   sigmoid(-40) = 4.2e-18 is an ordinary float32 (as it is in torch's float32 sigmoid), NOT zero: the outputs are
                 tiny and positive, the gradients of order 1e-17, all finite
    float32 o (1 - o) is exactly 0 in the first two where float64 keeps 1e-17 or less, so a relative comparison with float64
    means nothing here: the absolute error of each gradient is held against 1e-5 x the largest entry of the same gradient in
    float64 with b2 = 0 on the same inputs, and the output's against 1e-5 of the sigmoid's range."""
    x, w, go = _head_case(rows, b2=b2, w2_scale=0.1)
    got, ref, ref0 = _head_run(x, w, go), _head_reference(x, w, go), _head_reference(x, w, go, b2=0.0)
    for name, a in zip(HEAD_NAMES, got):
        assert torch.isfinite(a).all(), name
    if b2 != -40.0:
        exact = 1.0 if b2 > 0 else 0.0
        assert torch.equal(ref[0].float(), torch.full_like(got[0], exact))       # (float64 rounds there as well)
        assert torch.equal(got[0], torch.full_like(got[0], exact))
        for name, a in zip(HEAD_NAMES[1:], got[1:]):
            assert not a.any(), name
    else:
        assert bool((got[0] > 0).all()) and float(got[0].max()) <= 1e-12
    assert float((got[0].double() - ref[0]).abs().max()) <= 1e-5
    worst = {}
    for name, a, b, b0 in zip(HEAD_NAMES[1:], got[1:], ref[1:], ref0[1:]):
        worst[name] = float((a.double() - b).abs().max() / b0.abs().max())
    print(f'collision_head64 saturated rows={rows} b2={b2:g}:', {k: f'{v:.1e}' for k, v in worst.items()})
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.parametrize('rows', HEAD_SIZES)
def test_head64_bwd_acc_accumulates_into_existing_gradients(rows):
    """piml_head64_bwd_acc called directly, the struct built as _CollisionHead64.backward builds it from a forward run with
    `hidden`: accumulate = 0 overwrites `grads` (prefilled with NaN) and equals the operator's gradients bit for bit;
    accumulate = 1 on random values gives prefill + that result.  The slot sum is finished first and the old value added to it
    once (slot_sum_store, pack.hpp): ONE float32 addition, asserted bitwise.  The partial layout's pad floats are summed as
    zeros: they stay as prefilled."""
    from piml_amd import _lib, ops
    L = _lib.lib()
    x, w, go = _head_case(rows)
    full = _head_run(x, w, go)
    x2, wb = x.detach(), [t.detach() for t in w]
    opt = dict(device=x2.device, dtype=torch.float32)
    out, hidden, gx = torch.empty(rows, **opt), torch.empty(rows, 64, **opt), torch.empty(rows, 64, **opt)
    part = L.piml_head64_partial_floats()
    assert part == 64 * 64 + 64 + 64 + 4
    partials = torch.empty(L.piml_head64_slots(rows), part, **opt)
    H = _lib.Head64()
    H.x, H.rows = x2.data_ptr(), rows
    H.w1, H.b1, H.w2, H.b2 = [t.data_ptr() for t in wb]
    H.hidden, H.out = hidden.data_ptr(), out.data_ptr()
    _lib.check(L.piml_head64_fwd(ctypes.byref(H), ops._stream()), 'piml_head64_fwd')
    H.g_out, H.g_x, H.partials = go.data_ptr(), gx.data_ptr(), partials.data_ptr()
    fresh = torch.full((part,), float('nan'), **opt)
    H.grads = fresh.data_ptr()
    _lib.check(L.piml_head64_bwd_acc(ctypes.byref(H), 0, ops._stream()), 'piml_head64_bwd_acc')
    prefill = torch.randn(part, generator=torch.Generator().manual_seed(3)).to(DEV)
    acc = prefill.clone()
    H.grads = acc.data_ptr()
    _lib.check(L.piml_head64_bwd_acc(ctypes.byref(H), 1, ops._stream()), 'piml_head64_bwd_acc')
    torch.cuda.synchronize()
    assert torch.equal(out, full[0]) and torch.equal(gx, full[1])
    for name, a, b in zip(HEAD_NAMES[2:], (fresh[:4096], fresh[4096:4160], fresh[4160:4224], fresh[4224:4225]), full[2:]):
        assert torch.equal(a, b.flatten()), name
    assert not fresh[4225:].any()
    assert torch.equal(acc, prefill + fresh)
    assert torch.equal(acc[4225:], prefill[4225:])
    assert bool((acc[:4225] != prefill[:4225]).any())
