"""GPU: ops.fused_row_decoder (piml_rowdecoder_fwd / _bwd_acc, piml_amd/csrc/decoder.hip) where its dispatch turns -- the
1024-tile threshold between the workgroup-per-tile and the wave-per-tile kernels, the dW slab rule at 16 384 and 65 536 rows,
the clamps of the workgroup split, one branch alone on the many-rows kernels, three tiles to a wave -- and with upstream
gradients absent, weight gradients accumulated over the passes of a ParamGradSink step, deferred slot sums, a replayed graph
and refused arguments.  The shapes and what each reaches are rowdec_shapes.py's (preconditions: test_rowdec_shapes.py, and
again here before a launch); the reference is the float64 expression relu(e W1^T + b1) W2^T + b2, then . W3^T + b3,
differentiated by torch.autograd, every tensor held on its own to 1e-5 of the reference tensor's max-abs (the bound of
test_fused_row_decoder_matches_float64) -- the row-indexed ones again over the last tile and the last dW slab of a branch,
on those rows' own scale.  The two cases past the row counts that bound was measured at are held to max(1e-5, 4 x the error
of the same expression in plain float32 torch ops): a different summation order, not a dropped or doubled chunk.

Measured on an MI355X (worst entry of a case over its tensors and windows, split bf16 products / f32 instruction):
at_threshold 6.4e-7 (the few-rows kernels in both modes), over_threshold 3.8e-7 / 6.0e-7, slot_cap 2.3e-7 / 4.4e-7,
past_slot_cap 3.2e-7 / 4.7e-7, lopsided 7.9e-7 / 1.0e-6, one_branch_small 3.3e-7, one_branch_over 5.4e-7 / 6.5e-7,
live_subset 5.4e-7 / 7.2e-7.  one_branch_long: 3.1e-7 / 8.4e-7, float32 torch ops 2.8e-7 .. 4.0e-7 on the row-indexed
tensors and the biases, 3.6e-6 .. 3.8e-6 on dW1, dW2, dW3 -- bounds 1.44e-5, 1.50e-5, 1.48e-5 there, 1e-5 elsewhere.
two_long: 2.2e-7 / 7.0e-7, float32 torch ops 1.6e-6 .. 3.4e-6 on the dW -- bounds 1.12e-5 / 1.14e-5 (dW1), 1e-5 / 1.38e-5
(dW2), 1e-5 elsewhere.  Three accumulated passes: 4.1e-7 / 6.4e-7."""
import contextlib
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import rowdec_shapes as SH  # noqa: E402
from test_encoder_gpu import DEV, rowdec_products  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FIELDS = ('d emb', 'dW1', 'db1', 'dW2', 'db2', 'dW3', 'db3')
ROW_INDEXED = ('pred', 'decoded', 'd emb')
INVALID_VALUE = 1          # hipErrorInvalidValue

# which upstream gradients reach which branch, and which leaves ask for a gradient
VARIANTS = {
    'both': dict(),
    'pred_only': dict(mask=(True, False)),
    'decoded_only': dict(mask=(False, True)),              # g_pred absent: the operator's read-only zeros
    'emb_no_grad': dict(emb_grad=False),
    'weights_no_grad': dict(w_grad=False),
    'without_branch_0': dict(live=(1,)),
    'without_branch_1': dict(live=(0,)),
}


@functools.lru_cache(maxsize=None)
def device_inputs(name, extra=0):
    """the case's inputs on the device: [(emb, ws)] per branch, the upstream sets, the rows the guard replaced; callers
    leave them unchanged"""
    branches, ups = SH.make_inputs(name, extra)
    return ([(br['emb'].to(DEV), [w.to(DEV) for w in br['ws']]) for br in branches],
            [[(gp.to(DEV), gd.to(DEV)) for gp, gd in up] for up in ups], [br['replaced'] for br in branches])


def upstreams(name, variant, k=0, extra=0):
    v = VARIANTS[variant]
    mask, live = v.get('mask', (True, True)), v.get('live')
    return [None if live is not None and b not in live else tuple(g if m else None for g, m in zip(up, mask))
            for b, up in enumerate(device_inputs(name, extra)[1][k])]


def preconditions(name):
    """the case still reaches what it was chosen for, by the restated dispatch and by the library; and its guard stayed a guard"""
    from piml_amd import _lib
    c = SH.CASES[name]
    for key, value in SH.facts(c['rows']).items():
        assert c[key] == value, (name, key, value)
    for r, n in zip(c['rows'], c['slots']):
        assert _lib.lib().piml_rowdecoder_slots(r) == n, (name, r)
    for r, replaced in zip(c['rows'], device_inputs(name)[2]):
        assert replaced <= SH.guard_cap(r), (name, r, replaced)


def leaves_of(name, dtype, emb_grad=True, w_grad=True):
    return [[e.detach().to(dtype).requires_grad_(emb_grad)] + [w.detach().to(dtype).requires_grad_(w_grad) for w in ws]
            for e, ws in device_inputs(name)[0]]


def expression(lv):
    e, w1, b1, w2, b2, w3, b3 = lv
    d = torch.relu(e @ w1.t() + b1) @ w2.t() + b2
    return d @ w3.t() + b3, d


def fused(leaves):
    from piml_amd import ops
    return ops.fused_row_decoder([dict(emb=lv[0], decoder=lv[1:5], predictor=lv[5:]) for lv in leaves])


def loss_of(outs, ups):
    """sum over the branches with an upstream set of <pred, g_pred> + <decoded, g_decoded>, each where given"""
    terms = [(o * g.to(o.dtype)).sum() for out, up in zip(outs, ups) if up is not None for o, g in zip(out, up) if g is not None]
    return functools.reduce(lambda a, b: a + b, terms)


def results(outs, leaves, grads):
    """'<field> <branch>' -> tensor (None: autograd found no path to it); leaves that ask for no gradient have no entry"""
    res, it = {}, iter(grads)
    for b, (out, lv) in enumerate(zip(outs, leaves)):
        res[f'pred {b}'], res[f'decoded {b}'] = out[0].detach(), out[1].detach()
        for field, t in zip(FIELDS, lv):
            if t.requires_grad:
                res[f'{field} {b}'] = next(it)
    return res


def run(name, variant, dtype=None, k=0, extra=0):
    """forward and backward of a case: the fused operator (dtype None), or the expression in torch ops of `dtype`"""
    v = VARIANTS[variant]
    leaves = leaves_of(name, dtype or torch.float32, v.get('emb_grad', True), v.get('w_grad', True))
    outs = fused(leaves) if dtype is None else [expression(lv) for lv in leaves]
    wanted = [t for lv in leaves for t in lv if t.requires_grad]
    grads = torch.autograd.grad(loss_of(outs, upstreams(name, variant, k, extra)), wanted, allow_unused=True)
    return results(outs, leaves, grads)


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """float64, made once per case and variant; callers leave it unchanged"""
    return run(name, variant, torch.float64)


def errors(got, want, rows):
    """per tensor max |got - want| / max |want|; the row-indexed tensors also over the last tile and the last slab of their
    branch, relative to the reference's max-abs over those rows.  A tensor the reference has no path to is None or zero."""
    err = {}
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if w is None:
            assert g is None or not bool(g.any()), key
            continue
        assert g is not None and g.shape == w.shape and bool(torch.isfinite(g).all()), key
        diff = (g.double() - w).abs()
        err[key] = float(diff.max() / w.abs().max())
        field, b = key.rsplit(' ', 1)
        if field in ROW_INDEXED:
            for window, (r0, r1) in SH.row_windows(rows[int(b)]).items():
                err[f'{key} [{window}]'] = float(diff[r0:r1].max() / w[r0:r1].abs().max())
    return err


@functools.lru_cache(maxsize=None)
def bounds(name, variant='both'):
    """entry of errors() -> bound.  1e-5 where the project holds the operator to it already; past those row counts the error
    of plain float32 torch ops against float64 is the yardstick: max(1e-5, 4 x it) per entry"""
    if name not in SH.LONG:
        return None, {}
    yard = errors(run(name, variant, torch.float32), reference(name, variant), SH.CASES[name]['rows'])
    return yard, {k: max(SH.BOUND, 4.0 * v) for k, v in yard.items()}


def hold(tag, name, err, variant='both'):
    yard, bound = bounds(name, variant)
    worst = {}
    for key, e in err.items():
        field = key.split(' ', 1)[0] if not key.startswith('d emb') else 'd emb'
        worst[field] = max(worst.get(field, 0.0), e)
    print(f'\n[rowdec] {tag}: ' + ', '.join(f'{f} {e:.1e}' for f, e in worst.items()))
    if yard is not None:
        for key, e in err.items():
            print(f'[rowdec] {tag}: {key}: device {e:.2e}, float32 torch ops {yard[key]:.2e}, bound {bound[key]:.2e}')
    for key, e in err.items():
        assert e <= bound.get(key, SH.BOUND), (tag, key, e, bound.get(key, SH.BOUND))


def bitwise(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        assert bitwise(got[key], want[key]), (what, key)


def paths_tag(name, products, rows=None):
    fwd, dx, dw = SH.paths(rows or SH.CASES[name]['rows'], products)
    return f'{name} {SH.CASES[name]["rows"]} ({products}: {fwd}, {dx}, {dw})'


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(SH.CASES))
def test_case_matches_float64(name, rowdec_products):
    """both outputs and the seven gradients of every branch, upstream gradients on both outputs; twice, bitwise the same"""
    preconditions(name)
    want = reference(name, 'both')
    got = run(name, 'both')
    hold(paths_tag(name, rowdec_products), name, errors(got, want, SH.CASES[name]['rows']))
    same(run(name, 'both'), got, name)


@pytest.mark.parametrize('name,variant', [(n, v) for n in ('over_threshold', 'one_branch_small')
                                          for v in ('pred_only', 'decoded_only', 'emb_no_grad', 'weights_no_grad')])
def test_absent_gradients_match_float64(name, variant, rowdec_products):
    """a loss on one of the two outputs only (g_d2 a null pointer in the dX kernels / g_pred the operator's zeros), and leaves
    that ask for no gradient, on the many-rows kernels and on the few-rows ones"""
    preconditions(name)
    want = reference(name, variant)
    got = run(name, variant)
    asked = {k.split(' ')[0] if not k.startswith('d emb') else 'd emb' for k in got}
    assert ('d emb' in asked) == (variant != 'emb_no_grad') and ('dW1' in asked) == (variant != 'weights_no_grad')
    hold(f'{paths_tag(name, rowdec_products)} {variant}', name, errors(got, want, SH.CASES[name]['rows']))


@pytest.mark.parametrize('variant', ['without_branch_0', 'without_branch_1'])
def test_backward_of_one_live_branch_matches_float64(variant, rowdec_products):
    """the loss leaves a branch out: its leaves get None, and the backward launches the live branch alone -- branch 0 as ONE
    branch on the many-rows kernels, branch 1 on the few-rows kernels with the h1 / d2 of the many-rows forward"""
    name = 'live_subset'
    preconditions(name)
    rows = SH.CASES[name]['rows']
    live = VARIANTS[variant]['live'][0]
    assert SH.many_rows(rows) and SH.many_rows((rows[0],)) and not SH.many_rows((rows[1],))
    want = reference(name, variant)
    got = run(name, variant)
    for field in FIELDS:
        assert got[f'{field} {1 - live}'] is None and want[f'{field} {1 - live}'] is None, field
        assert got[f'{field} {live}'] is not None, field
    tag = f'{paths_tag(name, rowdec_products)} {variant}, backward {SH.paths((rows[live],), rowdec_products)[1:]}'
    hold(tag, name, errors(got, want, rows))


def _sink_step(name, passes, defer=False):
    """.grad of every leaf after the backward passes of one ParamGradSink step (passes: upstream sets as loss_of takes them)"""
    from piml_amd import ops
    leaves = leaves_of(name, torch.float32)
    sink = ops.ParamGradSink()
    with sink.step():
        with (ops.deferred_slot_sums() if defer else contextlib.nullcontext()):
            for ups in passes:
                loss_of(fused(leaves), ups).backward()
    torch.cuda.synchronize()
    return {f'{field} {b}': t.grad for b, lv in enumerate(leaves) for field, t in zip(FIELDS, lv)}


@pytest.mark.parametrize('mixed', [False, True], ids=['both_branches', 'first_pass_branch_1_only'])
def test_sink_accumulates_on_the_many_rows_path(mixed, rowdec_products):
    """three passes of one step with different upstream gradients: rowdec_reduce_kernel with `accumulate` on 256-row slabs.
    mixed: the first pass feeds the loss through branch 1 only, so the second finds branch 0's buffer new and branch 1's
    summed (ParamGradSink.take clears the new one on the host and the launch accumulates into both)."""
    name = 'over_threshold'
    preconditions(name)
    passes = [upstreams(name, 'without_branch_0' if mixed and k == 0 else 'both', k, extra=2) for k in range(3)]
    leaves = leaves_of(name, torch.float64)
    outs = [expression(lv) for lv in leaves]
    total = functools.reduce(lambda a, b: a + b, [loss_of(outs, ups) for ups in passes])
    grads = torch.autograd.grad(total, [t for lv in leaves for t in lv])
    want = {k: v for k, v in results(outs, leaves, grads).items() if not k.startswith(('pred', 'decoded'))}
    got = _sink_step(name, passes)
    assert set(got) == set(want)
    err = {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in want}
    hold(f'{paths_tag(name, rowdec_products)} sink, three passes, mixed {mixed}', name, err)


def test_deferred_slot_sums_are_bitwise_the_stand_alone_launch(rowdec_products):
    """inside ops.deferred_slot_sums() the slot sums of the many-rows backward are left to the block (PIML_DEFER_SLOT_SUMS):
    one pass, two passes, and two accumulating passes of a sink step give the gradients of the stand-alone launches"""
    from piml_amd import ops
    name = 'over_threshold'
    preconditions(name)
    alone = [run(name, 'both', k=k, extra=2) for k in range(2)]
    for passes in (1, 2):
        with ops.deferred_slot_sums():
            got = [run(name, 'both', k=k, extra=2) for k in range(passes)]
        torch.cuda.synchronize()
        for k in range(passes):
            same(got[k], alone[k], ('deferred', passes, k))
    ups = [upstreams(name, 'both', k, extra=2) for k in range(2)]
    same(_sink_step(name, ups, defer=True), _sink_step(name, ups), 'deferred under a sink step')


def test_captured_forward_and_backward_replay_bitwise(rowdec_products):
    """forward and backward on the many-rows kernels captured into a graph (one chain of launches) and replayed"""
    name = 'over_threshold'
    preconditions(name)
    leaves = leaves_of(name, torch.float32)
    ups = upstreams(name, 'both')
    flat = [t for lv in leaves for t in lv]

    def step():
        outs = fused(leaves)
        return [o for out in outs for o in out] + list(torch.autograd.grad(loss_of(outs, ups), flat))
    want = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = [t.detach() for t in step()]
    for _ in range(2):
        with torch.no_grad():
            for t in got:
                t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bitwise(a, b), i


# ---------------------------------------------------------------------------------------------------------------------

def _branch(rows, bwd):
    """a piml_decoder_branch of `rows` rows whose every pointer is a tensor's (kept alive beside it)"""
    from piml_amd import _lib
    L = _lib.lib()
    opt = dict(device=DEV, dtype=torch.float32)
    t = dict(msgs=torch.zeros(rows, 128, **opt), w1=torch.zeros(64, 128, **opt), b1=torch.zeros(64, **opt),
             w2=torch.zeros(64, 64, **opt), b2=torch.zeros(64, **opt), w3=torch.zeros(2, 64, **opt), b3=torch.zeros(2, **opt),
             h1=torch.zeros(rows, 64, **opt), d2=torch.zeros(rows, 64, **opt), pred=torch.zeros(rows, 2, **opt),
             packed=torch.zeros(L.piml_decoder_pack_floats(), **opt))
    if bwd:
        t.update(g_pred_rows=torch.zeros(rows, 2, **opt), g_pre2=torch.zeros(rows, 64, **opt), g_pre1=torch.zeros(rows, 64, **opt),
                 g_pooled=torch.zeros(rows, 128, **opt), grads=torch.zeros(L.piml_decoder_partial_floats(), **opt),
                 partials=torch.zeros(L.piml_rowdecoder_slots(rows), L.piml_decoder_partial_floats(), **opt))
    B = _lib.DecoderBranch()
    B.agents, B.k = rows, 1
    for field, tensor in t.items():
        setattr(B, field, tensor.data_ptr())
    return B, t


def test_entry_points_refuse_bad_arguments():
    """every refusal comes from the entry's own checks, in front of any launch: only null pointers and live tensors go in"""
    from piml_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    assert L.piml_rowdecoder_slots(0) == 0 and L.piml_rowdecoder_slots(-5) == 0
    entries = {'fwd': (lambda arr, n: L.piml_rowdecoder_fwd(arr, n, stream), False),
               'fwd_packed': (lambda arr, n: L.piml_rowdecoder_fwd_packed(arr, n, stream), False),
               'bwd_acc': (lambda arr, n: L.piml_rowdecoder_bwd_acc(arr, n, 0, stream), True)}
    with torch.cuda.device(DEV):
        for what, (call, bwd) in entries.items():
            made = [_branch(64, bwd) for _ in range(3)]
            good = lambda n=3: (_lib.DecoderBranch * n)(*[m[0] for m in made[:n]])     # noqa: E731
            assert call(good(), 0) == INVALID_VALUE, what
            assert call(good(), 3) == INVALID_VALUE, what
            assert call(None, 1) == INVALID_VALUE, what
            spoil = {'agents': 0, 'h1': None}
            spoil['partials' if bwd else 'pred'] = None
            for field, value in spoil.items():
                for nbr, at in ((1, 0), (2, 1)):
                    arr = good(nbr)
                    setattr(arr[at], field, value)
                    assert call(arr, nbr) == INVALID_VALUE, (what, field, nbr)
        torch.cuda.synchronize()
