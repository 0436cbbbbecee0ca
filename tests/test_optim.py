"""CPU: piml_amd.optim.Adam with a closure on CPU parameters is torch.optim.Adam's own step, bitwise, and never touches the HIP
library (the one launch serves device parameters only; tests/test_optim_gpu.py holds the device cases)."""
import pytest
import torch


def _no_library():
    raise AssertionError('piml_amd.optim.Adam reached the HIP library for CPU parameters')


def _model(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((7, 3), (3,), (1,), (1025,))]


@pytest.mark.parametrize('kw', [dict(lr=1e-2), dict(lr=3e-3, weight_decay=1e-2, betas=(0.8, 0.95)), dict(lr=1e-2, amsgrad=True)])
def test_closure_on_cpu_parameters_is_torchs_adam(monkeypatch, kw):
    from piml_amd import optim
    monkeypatch.setattr(optim._lib, 'lib', _no_library)
    mine, ref = _model(1), _model(1)
    x = torch.randn(16, 7, generator=torch.Generator().manual_seed(2))
    oa, ob = optim.Adam(mine, **kw), torch.optim.Adam(ref, **kw)

    def closure_for(opt, ps, calls):
        def closure():
            opt.zero_grad(set_to_none=True)
            w, b, c, v = ps
            loss = ((torch.tanh(x @ w + b) * c).square().sum() + (v * v.flip(0)).sum() * 1e-3)
            loss.backward()
            calls.append(loss)
            return loss
        return closure
    ca, cb = [], []
    fa, fb = closure_for(oa, mine, ca), closure_for(ob, ref, cb)
    for it in range(5):
        la, lb = oa.step(fa), ob.step(fb)
        assert len(ca) == it + 1 and len(cb) == it + 1, 'the closure runs exactly once per step()'
        assert la is ca[-1] and torch.equal(la, lb), it
        for p, q in zip(mine, ref):
            assert torch.equal(p, q), (it, tuple(p.shape))
    sa, sb = oa.state_dict()['state'], ob.state_dict()['state']
    assert sa.keys() == sb.keys()
    for k in sb:
        for name in sb[k]:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)
