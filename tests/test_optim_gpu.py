"""GPU: piml_amd.optim.Adam against torch.optim.Adam with the same constructor arguments and the same gradients, beyond the one
configuration the training loops use (tests/test_losses_gpu.py: one group of 15 tensors, fused=True, capturable=True, no closure):
parameters, exp_avg, exp_avg_sq and step BITWISE after every step (NaN masks equal, every other element bitwise), and every case
asserts which path ran -- the one launch (piml_adam_step) or torch's own step."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG = 3 * 2 ** 20 + 7          # ~3000 workgroups on one ticket


class _CountingLib:
    """the loaded library with its piml_adam_step calls counted"""

    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name != 'piml_adam_step':
            return f

        def counted(*a):
            self.calls += 1
            return f(*a)
        return counted


@pytest.fixture
def lib(monkeypatch):
    from piml_amd import optim
    proxy = _CountingLib(optim._lib.lib())
    monkeypatch.setattr(optim._lib, 'lib', lambda: proxy)
    return proxy


def bitwise(a, b, what):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, what
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), what
    x, y = a[~na], b[~nb]
    if x.dtype == torch.float32:
        x, y = x.view(torch.int32), y.view(torch.int32)
    assert torch.equal(x, y), what


def same_optimisers(oa, ob, mine, ref, what):
    for i, (p, q) in enumerate(zip(mine, ref)):
        bitwise(p, q, (what, i, 'param'))
        assert (p in oa.state) == (q in ob.state), (what, i)
        sa, sb = oa.state.get(p, {}), ob.state.get(q, {})
        assert sorted(sa) == sorted(sb), (what, i)
        for name in sb:
            bitwise(sa[name], sb[name], (what, i, name))


def params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    mine = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.2).to(DEV)) for n in sizes]
    return mine, [torch.nn.Parameter(p.detach().clone()) for p in mine]


def give_grads(mine, ref, g, it, skip=()):
    for i, (p, q) in enumerate(zip(mine, ref)):
        if i in skip:
            continue
        gr = (torch.randn(p.shape, generator=g) * (10.0 ** (it % 3 - 2))).to(DEV)
        p.grad, q.grad = gr, gr.clone()


@pytest.mark.parametrize('with_empty', [False, True])
def test_a_table_past_one_launch_in_two_groups(lib, with_empty):
    """90 tensors (three launches of at most 40 in the first group: the ticket buffer is reused across them), sizes around the
    1024-element piece and one of ~3000 workgroups, two groups with different hyper-parameters, a few parameters without a
    gradient (they do not move and get no state), 10 steps"""
    from piml_amd.optim import Adam
    pool = [1, 1023, 1024, 1025] + ([0] if with_empty else [])
    sizes = [pool[i % len(pool)] for i in range(90)]
    sizes[7] = sizes[61] = BIG
    mine, ref = params(sizes, seed=1)
    nograd = {3, 44, 88}
    groups = lambda ps: [dict(params=ps[:84], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
                         dict(params=ps[84:], lr=3e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)]
    kw = dict(fused=True, capturable=True)
    oa, ob = Adam(groups(mine), **kw), torch.optim.Adam(groups(ref), **kw)
    g = torch.Generator().manual_seed(2)
    for it in range(10):
        give_grads(mine, ref, g, it, skip=nograd)
        oa.step()
        ob.step()
        assert lib.calls == 2 * (it + 1)          # one call per group
        same_optimisers(oa, ob, mine, ref, it)
    for i in nograd:
        assert mine[i] not in oa.state and ref[i] not in ob.state


def test_an_empty_parameter_steps_its_counter(lib):
    """zero-element parameters with a gradient: the caching allocator gives them null data pointers; torch steps their counter"""
    from piml_amd.optim import Adam
    mine, ref = params([0, 5, 0, 1030], seed=3)
    assert mine[0].data_ptr() == 0, 'the caching allocator gives an empty tensor a null pointer: the case under test'
    kw = dict(lr=1e-2, fused=True, capturable=True)
    oa, ob = Adam(mine, **kw), torch.optim.Adam(ref, **kw)
    g = torch.Generator().manual_seed(4)
    for it in range(3):
        give_grads(mine, ref, g, it)
        oa.step()
        ob.step()
        assert lib.calls == it + 1
        same_optimisers(oa, ob, mine, ref, it)
    assert float(oa.state[mine[0]]['step']) == 3.0


GRID = [dict(fused=f, capturable=c, weight_decay=wd) for f in (True, None) for c in (True, False) for wd in (0.0, 1e-2)] + [
    dict(fused=True, capturable=True, amsgrad=True), dict(fused=True, capturable=True, maximize=True),
    dict(fused=None, capturable=True, amsgrad=True, weight_decay=1e-2), dict(fused=None, capturable=False, maximize=True),
    dict(fused=None, foreach=False), dict(fused=None, foreach=False, capturable=True), dict(fused=True, foreach=False)]


@pytest.mark.parametrize('kw', GRID, ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_configuration_grid(lib, kw):
    """the one launch runs exactly when the group asks for the fused step (and nothing else rules it out); every other
    configuration is torch's own step, with torch's own arithmetic"""
    from piml_amd.optim import Adam
    mine, ref = params([1, 1023, 1024, 1025, 5000], seed=5)
    kw = dict(lr=2e-3, **kw)
    try:
        ob = torch.optim.Adam(ref, **kw)
    except (RuntimeError, ValueError) as e:
        pytest.skip(f'torch refuses {kw}: {e}')
    oa = Adam(mine, **kw)
    launch = bool(kw.get('fused')) and not kw.get('amsgrad') and not kw.get('maximize')
    g = torch.Generator().manual_seed(6)
    for it in range(4):
        give_grads(mine, ref, g, it)
        oa.step()
        ob.step()
        assert lib.calls == (it + 1 if launch else 0), kw
        same_optimisers(oa, ob, mine, ref, it)


@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_gradient_edges(lib, wd):
    """exact zeros, subnormals, magnitudes whose square overflows float32, isolated inf and nan -- one tensor of each, plus one
    with all of them side by side across two workgroups"""
    from piml_amd.optim import Adam
    n = 1100
    mine, ref = params([n] * 6, seed=7)
    kw = dict(lr=1e-3, weight_decay=wd, fused=True, capturable=True)
    oa, ob = Adam(mine, **kw), torch.optim.Adam(ref, **kw)
    g = torch.Generator().manual_seed(8)
    sign = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    for it in range(3):
        base = torch.randn(n, generator=g) * 1e-2
        zeros = torch.zeros(n)
        sub = sign() * 1e-40 * (1 + torch.rand(n, generator=g))
        huge = sign() * 1e30 * (1 + torch.rand(n, generator=g))
        inf = base.clone(); inf[[5, 1030]] = float('inf'); inf[700] = -float('inf')
        nan = base.clone(); nan[[17, 1099]] = float('nan')
        mixed = base.clone()
        for lo, src in zip((0, 200, 400, 1020), (zeros, sub, huge, huge)):
            mixed[lo:lo + 100] = src[lo:lo + 100]
        mixed[650], mixed[1050], mixed[1051] = float('inf'), float('nan'), -float('inf')
        assert sub.abs().max() < torch.finfo(torch.float32).tiny and (sub != 0).all()
        for p, q, gr in zip(mine, ref, (zeros, sub, huge, inf, nan, mixed)):
            p.grad, q.grad = gr.to(DEV), gr.to(DEV)
        oa.step()
        ob.step()
        assert lib.calls == it + 1
        same_optimisers(oa, ob, mine, ref, it)


@pytest.mark.parametrize('fused', [True, None])
def test_counters_near_the_float32_limit(lib, fused):
    """step = 2^24 - 3, then 5 steps: the float32 counter saturates at 2^24 in both, and the bias corrections there agree"""
    from piml_amd.optim import Adam
    mine, ref = params([1, 1025, 4096], seed=9)
    kw = dict(lr=1e-3, betas=(0.5, 0.9999), fused=fused, capturable=True)
    oa, ob = Adam(mine, **kw), torch.optim.Adam(ref, **kw)
    g = torch.Generator().manual_seed(10)
    give_grads(mine, ref, g, 0)
    oa.step()
    ob.step()
    for o in (oa, ob):
        for st in o.state.values():
            st['step'].fill_(2 ** 24 - 3)
    for it in range(5):
        give_grads(mine, ref, g, it + 1)
        oa.step()
        ob.step()
        same_optimisers(oa, ob, mine, ref, it)
    assert lib.calls == (6 if fused else 0)
    assert all(float(st['step']) == 2.0 ** 24 for st in oa.state.values())


def _closure_for(opt, ps, x, calls):
    def closure():
        opt.zero_grad(set_to_none=True)
        loss = sum((torch.tanh(p * x[:p.numel()]) * (i + 1)).square().sum() for i, p in enumerate(ps))
        loss.backward()
        calls.append(loss)
        return loss
    return closure


@pytest.mark.parametrize('fallback_group', [False, True])
def test_closure(lib, fallback_group):
    """the usual closure (zero_grad(set_to_none=True), forward, backward): evaluated once per step() BEFORE the gradients are
    gathered, its value returned; with one group on torch's step (amsgrad) the whole step is torch's, the closure still once"""
    from piml_amd.optim import Adam
    mine, ref = params([1, 1023, 1025, 3000], seed=11)
    x = torch.randn(3000, generator=torch.Generator().manual_seed(12)).to(DEV)
    groups = lambda ps: [dict(params=ps[:2]), dict(params=ps[2:], amsgrad=fallback_group, lr=5e-3)]
    kw = dict(lr=1e-2, fused=True, capturable=True)
    oa, ob = Adam(groups(mine), **kw), torch.optim.Adam(groups(ref), **kw)
    ca, cb = [], []
    fa, fb = _closure_for(oa, mine, x, ca), _closure_for(ob, ref, x, cb)
    for it in range(5):
        la, lb = oa.step(fa), ob.step(fb)
        assert len(ca) == it + 1 and len(cb) == it + 1, 'the closure runs exactly once per step()'
        assert la is ca[-1]
        bitwise(la, lb, it)
        assert lib.calls == (0 if fallback_group else 2 * (it + 1))
        same_optimisers(oa, ob, mine, ref, it)
    assert all(float(st['step']) == 5.0 for st in oa.state.values())


def test_grad_scaler_goes_to_torchs_step(lib):
    """torch.amp.GradScaler drives the fused optimiser through its grad_scale / found_inf attributes: that is torch's step (the
    one launch does not unscale); an inf gradient skips the step and lowers the scale the same way"""
    from piml_amd.optim import Adam
    mine, ref = params([1, 1023, 1025], seed=13)
    kw = dict(lr=1e-2, fused=True, capturable=True)
    oa, ob = Adam(mine, **kw), torch.optim.Adam(ref, **kw)
    sa, sb = torch.amp.GradScaler('cuda', init_scale=2.0 ** 12), torch.amp.GradScaler('cuda', init_scale=2.0 ** 12)
    x = torch.randn(1025, generator=torch.Generator().manual_seed(14)).to(DEV)
    for it in range(4):
        before = [p.detach().clone() for p in mine]
        for o, s, ps in ((oa, sa, mine), (ob, sb, ref)):
            o.zero_grad(set_to_none=True)
            s.scale(sum(torch.tanh(p * x[:p.numel()]).square().sum() for p in ps)).backward()
            if it == 2:
                ps[1].grad[100] = float('inf')
            s.step(o)
            s.update()
        assert sa.get_scale() == sb.get_scale(), it
        same_optimisers(oa, ob, mine, ref, it)
        if it == 2:
            assert sa.get_scale() < 2.0 ** 12
            assert all(torch.equal(p, b) for p, b in zip(mine, before)), 'the scaler skips the step of an inf gradient'
    assert lib.calls == 0
