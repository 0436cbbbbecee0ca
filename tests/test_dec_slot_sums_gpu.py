"""GPU: the decoder's weight-gradient slots of the sums path (PIML_POOL_TRAIN, two-crew encoder backward) summed by the encoder
backward's workgroups, and the unfold of the folded first layers run as workgroups of the slot-sum launch
(piml_encoder_sums_dec_slots(1), the default) -- against the slot-sum launch summing them and the unfold as a launch of its own
(piml_encoder_sums_dec_slots(0)).  Same slots, same summation order (pack.hpp: slot_chains): every gradient BITWISE the same, for
ragged shapes, accumulating passes under a ParamGradSink step (deferred unfold), deferred slot sums and inside a replayed graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_sums_gpu import DEV, make_net, run  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0.5
SHAPES = [(4096, (6, 10), True), (2500, (6, 10), False), (4099, (10, 6), True), (12000, (6, 2), True), (3001, (2, 10), False)]


def _switch(on):
    from piml_amd import _lib
    return _lib.lib().piml_encoder_sums_dec_slots(1 if on else 0)


def _both(fn):
    """fn() with the decoder slots summed by the slot-sum launch (today's placement) and by the encoder backward"""
    old = _switch(False)
    try:
        off = fn()
        _switch(True)
        on = fn()
    finally:
        _switch(old)
    torch.cuda.synchronize()
    return off, on


def _bitwise(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(off, on, what):
    assert len(off) == len(on), what
    for i, (a, b) in enumerate(zip(off, on)):
        assert _bitwise(a, b), (what, i, float((a - b).abs().max()))


def test_switch_defaults_on():
    from piml_amd import _lib
    want = 0 if os.environ.get('PIML_ENC_DEC_SLOTS', '').strip() == '0' else 1
    assert _lib.lib().piml_encoder_sums_dec_slots(-1) == want


@pytest.mark.parametrize('agents,ks,with_head', SHAPES)
def test_one_pass_bitwise(agents, ks, with_head):
    brs, sf, head, wa, _ = make_net(agents, ks, with_head, seed=7)
    off, on = _both(lambda: [t.clone() for t in run(brs, sf, head, wa, TAU, True)[1]])
    _same(off, on, (agents, ks, with_head))


@pytest.mark.parametrize('agents,ks,with_head', SHAPES[:3])
def test_accumulating_passes_under_a_sink_step(agents, ks, with_head):
    """three backward passes of one optimiser step into a ParamGradSink's buffers: PIML_ACCUMULATE from the second pass on, the
    unfold deferred to the step's end (piml_pinnsf_unfold_defer) -- the slot-sum launches then carry no unfold workgroups"""
    from piml_amd import ops
    brs, sf, head, wa, g = make_net(agents, ks, with_head, seed=11)
    was = [torch.randn(wa.shape, generator=g).to(DEV) for _ in range(3)]
    leaves = [sf] + [t for br in brs for t in (br['x'], *br['encoder'], *br['decoder'], *br['predictor'])]

    def step():
        for t in leaves:
            t.grad = None
        sink = ops.ParamGradSink()
        with sink.step():
            for w in was:
                res = ops.fused_pinnsf(brs, sf, TAU, fold_epilogue=True, head=head, sums=True)
                (res[0] * w).sum().backward()
        out = [t.grad.clone() for t in leaves]
        for t in leaves:
            t.grad = None
        return out
    off, on = _both(step)
    _same(off, on, ('sink', agents, ks, with_head))


@pytest.mark.parametrize('agents,ks,with_head', SHAPES[:2])
def test_deferred_slot_sums_carry_the_unfold(agents, ks, with_head):
    """the slot sums left to the block's exit (ops.deferred_slot_sums): the stand-alone slot-sum launch with the unfold's
    workgroups in front; two passes in one block, the first one's sums flushed behind the second one's encoder backward"""
    from piml_amd import ops
    brs, sf, head, wa, g = make_net(agents, ks, with_head, seed=13)
    wa2 = torch.randn(wa.shape, generator=g).to(DEV)
    leaves = [sf] + [t for br in brs for t in (br['x'], *br['encoder'], *br['decoder'], *br['predictor'])]

    def step(passes):
        out = []
        with ops.deferred_slot_sums():
            for w in (wa, wa2)[:passes]:
                res = ops.fused_pinnsf(brs, sf, TAU, fold_epilogue=True, head=head, sums=True)
                out.append(torch.autograd.grad((res[0] * w).sum(), leaves))
        torch.cuda.synchronize()
        return [t.clone() for gr in out for t in gr]
    for passes in (1, 2):
        off, on = _both(lambda: step(passes))
        _same(off, on, ('deferred', passes, agents, ks))


def test_relfeat_backward_carries_the_unfold():
    """the model's step with the slot sums deferred into the relfeat backward's launch (its leading workgroups: the unfold's, then
    the slot sums'), once and twice in one block"""
    from test_deferred_sums_gpu import _model, _scene, _step
    model, scene = _model(), _scene()
    for twice in (False, True):
        off, on = _both(lambda: _step(model, scene, True, twice=twice))
        _same(off[:-1], on[:-1], ('relfeat', twice))
        assert torch.allclose(off[-1], on[-1], rtol=1e-5, atol=1e-6)      # d/d(state): float atomics, order not fixed


@pytest.mark.parametrize('agents,ks,with_head', [SHAPES[0], SHAPES[2]])
def test_captured_step_replays_bitwise(agents, ks, with_head):
    brs, sf, head, wa, _ = make_net(agents, ks, with_head, seed=17)
    old = _switch(False)
    try:
        want = [t.clone() for t in run(brs, sf, head, wa, TAU, True)[1]]
        _switch(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                run(brs, sf, head, wa, TAU, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, got = run(brs, sf, head, wa, TAU, True)
    finally:
        _switch(old)
    for _ in range(3):
        with torch.no_grad():
            for t in got:
                t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        _same(want, got, ('graph', agents, ks))
