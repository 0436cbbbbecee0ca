"""CPU-only: fuzz the oracle against the reference's own outputs on random small scenes (random k, sight angles,
thresholds), captured with their inputs in tests/golden/live_reference.npz (tests/golden/make_golden.py live_reference).
Widens the pinning of the oracle beyond the real-clip golden vectors; also the host-side rollout losses and the pointwise
data loader against the reference's."""
import numpy as np
import torch

from conftest import bits, golden


def test_relfeat_fuzz_oracle_equals_live_reference(oracle):
    g = golden('live_reference')
    n_cases = int(g['relfeat_cases'])
    assert n_cases == 120
    for case in range(n_cases):
        c = f'relfeat{case}/'
        p, v, a, d, o = (g[c + k] for k in ('position', 'velocity', 'acceleration', 'destination', 'obstacles'))
        kp, ang_p, dp, ko, ang_o, do = g[c + 'params']
        pf, of, df = oracle.relfeat_fwd(p, v, a, d, o, int(kp), ang_p, dp, int(ko), ang_o, do)
        # random continuous positions: no exact distance ties, so even the slot order must agree
        assert np.array_equal(bits(pf), bits(g[c + 'ped_features'])), (case, p.shape, o.shape, kp, ang_p, dp)
        assert np.array_equal(bits(of), bits(g[c + 'obs_features'])), (case, p.shape, o.shape, ko, ang_o, do)
        assert np.array_equal(bits(df), bits(g[c + 'dest_features']))


def test_rollout_losses_equal_live_reference():
    """The rollout losses of BaseSimulator (pure torch, host side) against the reference's methods' values."""
    from piml_amd.models.simulators import BaseSimulator as Mine
    g = golden('live_reference')
    T = lambda k: torch.from_numpy(g['losses/' + k])         # noqa: E731
    mine = Mine.__new__(Mine)
    pred, lab, coll, am = T('pred'), T('labels'), T('collisions'), T('abnormal_mask')
    for decay in (1.0, 0.9):
        for rev in (False, True):
            a = mine.multiple_rollout_mse_loss(pred, lab, decay, reduction='sum', reverse=rev)
            assert torch.allclose(a, T(f'mse_d{decay}_r{int(rev)}'), rtol=1e-6)
        a = mine.multiple_rollout_collision_avoidance_loss(pred, lab, decay, reduction='none')
        assert torch.allclose(a, T(f'avoid_d{decay}'), rtol=1e-5, atol=1e-7)
        for tag, mask in (('none', None), ('mask', am)):
            a = mine.multiple_rollout_collision_loss(pred, lab, decay, 10, coll.clone(), reduction='sum', abnormal_mask=mask)
            assert torch.allclose(a, T(f'coll_d{decay}_{tag}'), rtol=1e-5)
    assert torch.allclose(mine.l1_reg_loss(T('embedding'), 0.01, 'sum'), T('l1'))


def test_data_loader_equals_live_reference():
    """Same batches as the reference's loader for pointwise data under the same numpy seed."""
    from piml_amd.data.data import PointwisePedData
    from piml_amd.utils import data_loader as LOAD
    g = golden('live_reference')
    n = 23
    feats = dict(ped_features=torch.arange(n * 2 * 6.).reshape(n, 2, 6), obs_features=torch.zeros(n, 3, 6),
                 self_features=torch.arange(n * 7.).reshape(n, 7), labels=torch.arange(n * 12.).reshape(n, 12))
    mine = PointwisePedData()
    for k, v in feats.items():
        setattr(mine, k, v)
    mine.dataset_len = n
    np.random.seed(5)
    a = LOAD.data_loader(mine, 4, seed=0)
    assert len(a) == int(g['loader/batches']) == n // 4
    for i, x in enumerate(a):
        assert len(x) == int(g[f'loader/b{i}/fields'])
        for j, u in enumerate(x):
            w = torch.from_numpy(g[f'loader/b{i}/{j}'])
            assert u.dtype == w.dtype and torch.equal(u, w)
