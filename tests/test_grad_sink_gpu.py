"""GPU: the sums path (ops.fused_pinnsf(sums=True), PIML_POOL_TRAIN) while an ops.ParamGradSink step is open, outside the training
loops' happy path -- backward passes whose forward did NOT run under the step (they take the non-sink branch and hand fresh
buffers to autograd, so their unfold must run at once: PIML_DEFER_UNFOLD of piml_pinnsf_bwd), two networks under one step,
the loops' nesting with deferred slot sums, and an exception inside a step.  References: the same call outside any sink step
(bitwise: the same launches in the same order) and the float64 restatement of tests/test_sums_gpu.py (1e-5 of the tensor's
largest entry, the bar of test_sums_path_matches_float64_and_the_message_path)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_sums_gpu import DEV, dodge_relu_kinks, forward64, make_net, run  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0.5


def _net(seed):
    brs, sf, head, wa, g = make_net(4096, (6, 10), True, seed)
    dodge_relu_kinks(brs, sf, head, TAU, g)
    n = types.SimpleNamespace(brs=brs, sf=sf, head=head, wa=wa, wa2=torch.randn(wa.shape, generator=g).to(DEV))
    n.leaves = [sf] + [t for br in brs for t in (br['x'], *br['encoder'], *br['decoder'], *br['predictor'])]
    n.ref = [t.clone() for t in run(brs, sf, head, wa, TAU, True)[1]]
    acc64, _, leaves64, _ = forward64(brs, sf, head, TAU)
    n.ref64 = torch.autograd.grad((acc64 * wa.double()).sum(), leaves64)
    return n


@pytest.fixture(scope='module')
def nets():
    return _net(31), _net(32)


@pytest.fixture(autouse=True)
def no_grads(nets):
    for n in nets:
        for t in n.leaves + n.head:
            t.grad = None
    yield
    for n in nets:
        for t in n.leaves + n.head:
            t.grad = None


def loss_of(n, wa=None):
    from piml_amd import ops
    res = ops.fused_pinnsf(n.brs, n.sf, TAU, fold_epilogue=True, head=n.head, sums=True)
    return (res[0] * (n.wa if wa is None else wa)).sum()


def bitwise_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def check(n, got, what):
    assert len(got) == len(n.ref)
    for i, (a, r, r64) in enumerate(zip(got, n.ref, n.ref64)):
        assert bitwise_equal(a, r), (what, i, rel(a, r))
        assert rel(a, r64) <= 1e-5, (what, i)


def test_forward_before_the_step_autograd_grad_inside_it(nets):
    """the backward's forward ran before step(): the non-sink branch, whose gradients are read inside the still open step"""
    from piml_amd import ops
    A = nets[0]
    loss = loss_of(A)
    with ops.ParamGradSink().step():
        grads = torch.autograd.grad(loss, A.leaves)
        torch.cuda.synchronize()
        got = [g.clone() for g in grads]
    check(A, got, 'inside the step')


def test_existing_grads_accumulate_the_unfolded_gradients(nets):
    """every leaf holds a .grad G0: AccumulateGrad adds the pass's gradients inside the step, which must be unfolded by then"""
    from piml_amd import ops
    A = nets[0]
    g = torch.Generator().manual_seed(41)
    g0 = [torch.randn(t.shape, generator=g).to(DEV) for t in A.leaves]
    for t, x in zip(A.leaves, g0):
        t.grad = x.clone()
    loss = loss_of(A)
    with ops.ParamGradSink().step():
        loss.backward()
    torch.cuda.synchronize()
    for i, (t, x, r) in enumerate(zip(A.leaves, g0, A.ref)):
        assert bitwise_equal(t.grad, x + r), i


def test_freed_gradient_buffers_are_not_written_when_the_step_closes(nets):
    """the gradients of a non-sink pass are dropped inside the step; the blocks they lived in go to new tensors (sentinels), which
    the step's end must leave untouched.  (Never empty_cache() in here: a stray write has to land in the caching allocator's
    pool, where it corrupts a sentinel -- what this test detects -- and cannot reach unmapped memory.)"""
    from piml_amd import ops
    A = nets[0]
    loss = loss_of(A)
    sentinels = []
    with ops.ParamGradSink().step():
        grads = torch.autograd.grad(loss, A.leaves)
        del loss
        freed = {}
        for t in grads:
            freed[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
        del grads, t
        for i, (ptr, nbytes) in enumerate(sorted(freed.items())):
            s = torch.empty(nbytes // 4, device=DEV)
            s.fill_(1000.0 + i)
            sentinels.append(s)
        assert any(s.data_ptr() in freed for s in sentinels), 'no freed gradient buffer was handed out again: the test proves nothing'
    torch.cuda.synchronize()
    for i, s in enumerate(sentinels):
        assert bool((s == 1000.0 + i).all()), f'sentinel {i} ({s.numel()} floats) was written after its buffer was freed'


def _two_passes_each(A, B, sink):
    import contextlib
    for n in (A, B):
        for t in n.leaves:
            t.grad = None
    with (sink.step() if sink is not None else contextlib.nullcontext()):
        losses = [loss_of(A, A.wa), loss_of(B, B.wa), loss_of(A, A.wa2), loss_of(B, B.wa2)]
        for loss in losses:
            loss.backward()
    torch.cuda.synchronize()
    return [[t.grad.clone() for t in n.leaves] for n in (A, B)]


def test_two_networks_under_one_sink_step(nets):
    """two passes of each of two sums-path networks, interleaved, both under the sink: each network's deferred unfold is
    launched when the other's backward comes (network.hip: launch_unfold), the last at the step's end"""
    from piml_amd import ops
    A, B = nets
    want = _two_passes_each(A, B, None)
    sink = ops.ParamGradSink()
    got, again = _two_passes_each(A, B, sink), _two_passes_each(A, B, sink)
    for w, g, a in zip(want, got, again):
        for i, (x, y, z) in enumerate(zip(w, g, a)):
            assert bitwise_equal(y, z), i
            assert float((y - x).abs().max()) <= 2e-6 * float(x.abs().max()), (i, rel(y, x))


def test_the_loops_nesting_with_one_network_outside_the_sink(nets):
    """`with sink.step(), ops.deferred_slot_sums():` (the training loops' form, written as two blocks to look in between): A's
    forward inside the step, B's before it; B's slot sums are deferred to the inner block's exit and its unfold must not wait
    for the step's"""
    from piml_amd import ops
    A, B = nets
    lb = loss_of(B)
    with ops.ParamGradSink().step():
        with ops.deferred_slot_sums():
            la = loss_of(A)
            (la + lb).backward()
        torch.cuda.synchronize()
        got_b = [t.grad.clone() for t in B.leaves]
    torch.cuda.synchronize()
    check(B, got_b, 'B before the step closes')
    for i, (t, r) in enumerate(zip(A.leaves, A.ref)):
        assert float((t.grad - r).abs().max()) <= 2e-6 * float(r.abs().max()), (i, rel(t.grad, r))
        assert rel(t.grad, A.ref64[i]) <= 1e-5, i


class _Boom(Exception):
    pass


def test_an_exception_inside_a_step_leaks_no_deferral(nets):
    from piml_amd import ops
    A = nets[0]
    with pytest.raises(_Boom):
        with ops.ParamGradSink().step():
            loss_of(A).backward()
            raise _Boom()
    assert ops.ParamGradSink._active is None
    for t in A.leaves:
        t.grad = None
    _, grads = run(A.brs, A.sf, A.head, A.wa, TAU, True)
    torch.cuda.synchronize()
    check(A, grads, 'after the exception')
