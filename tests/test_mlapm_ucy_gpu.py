"""GPU: the UCY two-phase pair path (mlapm_tile_sum's 256-entry candidate ring; mlapm_bwd_kernel's and
mlapm_bwd_ucy_fix_kernel's 128-entry rings) against the float64 yardstick of tests/mlapm_ucy_ref.py, on scenes where the
rings fill, wrap and drain several times in a row, where pairs sit on the conservative filter's boundary, and where nothing
is a candidate at all.  tests/test_mlapm_ucy_ref.py asserts, without a GPU, that the scenes are what they are meant to be.

The bars are the project's own for this law (1e-5 forward, 2e-5 gradients), not measured ones.  Measured on an MI355X against
step64, for orientation: forward and skip_absent at most 2.9e-7 of m_i, gradients at most 3.4e-7 of the largest entry, over
all cases and both laws; the same law in float32 torch on the CPU is 1.4e-7 - 1.8e-7 from step64 in the forward measure."""
import numpy as np
import pytest
import torch

import mlapm_ucy_ref as R
from mlapm_direct import DEV, _mlapm_bwd_direct, dev

pytestmark = pytest.mark.gpu

DT, RADIUS = 0.08, 0.3
FWD_BAR = 1e-5        # the project's bar for this smooth law, of m_i = |v_i| + dt (|desired force_i| + sum_j |term_ij|)
GRAD_BAR = 2e-5       # ... for gradients, of the largest entry of each gradient tensor
LAWS = {'ucy': R.UCY_LAW, 'jump': R.JUMP_LAW}
KEYS = ('position', 'velocity', 'desired_speed', 'destination')
BWD_CASES = tuple(c for c in R.CASES if c != 'boundary')      # the reference's gradient is not defined at d^2 = 0
WS_CASES = ('clump700', 'clump2200')                          # N >= 512: the once-per-pair backward + mlapm_bwd_ucy_fix_kernel

_ref = {}


def upstream(N):
    return np.random.default_rng(1000 + N).standard_normal((N, 2)).astype(np.float32)


def reference(name, law):
    """step64 of a case with the seeded upstream gradient: computed once, shared, never written to"""
    if (name, law) not in _ref:
        sc = R.case(name)
        w = None if name == 'boundary' else upstream(sc['position'].shape[0])
        _ref[name, law] = R.step64(*[sc[k] for k in KEYS], LAWS[law], DT, RADIUS, w=w, device=DEV)
    return _ref[name, law]


def forward(sc, law, **kw):
    from piml_amd import ops
    return ops.mlapm_step(*[dev(sc[k]) for k in KEYS], DT, RADIUS, version='UCY', **LAWS[law], **kw).cpu().numpy()


def check_forward(tag, got, ref, rows=None):
    rows = np.ones(len(got), bool) if rows is None else rows
    assert np.isfinite(got[rows]).all(), tag
    ratio = np.linalg.norm(got[rows] - ref.action[rows], axis=-1) / np.maximum(ref.m[rows], 1e-3)
    print(f'{tag}: worst |got - ref| / max(m, 1e-3) = {ratio.max():.2e} at row {np.flatnonzero(rows)[ratio.argmax()]} (bar {FWD_BAR:g})')
    assert ratio.max() <= FWD_BAR, (tag, ratio.max())


def check_grads(tag, got, ref):
    worst = []
    for g, r, name in zip(got, ref.grads, ('gp', 'gv', 'gv0', 'gdest')):
        assert np.isfinite(g).all(), (tag, name)
        g, r = g.reshape(-1), r.reshape(-1)
        worst.append(np.abs(g - r).max() / max(np.abs(r).max(), 1e-3))
    print(f'{tag}: worst |got - ref| / max|ref| for gp, gv, gv0, gdest = ' + ', '.join(f'{x:.2e}' for x in worst) + f' (bar {GRAD_BAR:g})')
    assert max(worst) <= GRAD_BAR, (tag, worst)


@pytest.mark.parametrize('law', list(LAWS))
@pytest.mark.parametrize('name', R.CASES)
def test_forward_matches_float64(name, law):
    sc = R.case(name)
    check_forward(f'forward {name} {law}', forward(sc, law), reference(name, law))


@pytest.mark.parametrize('law', list(LAWS))
@pytest.mark.parametrize('name', BWD_CASES)
def test_two_role_backward_matches_float64_autograd(name, law):
    """piml_mlapm_step_bwd (mlapm_bwd_kernel) on every shape, the large ones included"""
    sc = R.case(name)
    w = dev(upstream(sc['position'].shape[0]))
    rc, got = _mlapm_bwd_direct('two_role', sc, w, 'UCY', law=LAWS[law])
    assert rc == 0
    check_grads(f'two-role backward {name} {law}', got, reference(name, law))


@pytest.mark.parametrize('law', list(LAWS))
@pytest.mark.parametrize('name', WS_CASES)
def test_workspace_backward_matches_float64_autograd(name, law):
    """piml_mlapm_step_bwd_ws: mlapm_bwd_sys_kernel<2> + mlapm_bwd_ucy_fix_kernel"""
    sc = R.case(name)
    w = dev(upstream(sc['position'].shape[0]))
    rc, got = _mlapm_bwd_direct('ws', sc, w, 'UCY', law=LAWS[law])           # (asserts a positive workspace size)
    assert rc == 0
    check_grads(f'workspace backward {name} {law}', got, reference(name, law))


def test_workspace_form_serves_exactly_the_large_shapes():
    from piml_amd import _lib, ops
    L = _lib.lib()
    for name in R.CASES:
        N = R.case(name)['position'].shape[0]
        need = int(L.piml_mlapm_bwd_workspace_floats(N, ops.MLAPM_VARIANTS['UCY']))
        assert (need > 0) == (name in WS_CASES) == (N >= 512), (name, N, need)


@pytest.mark.parametrize('law', list(LAWS))
@pytest.mark.parametrize('name', list(R.CLUMP_SHAPES) + ['boundary', 'sparse257_drift'])
def test_skip_absent_matches_the_compacted_scene(name, law):
    """10 % of the agents absent (NaN positions; index 0, the last index, inside and outside the clump): the rows of the
    present agents are the reference's step on the compacted scene; without skip_absent the NaNs poison every row."""
    sc = dict(R.case(name))
    gone = R.absent_mask(sc)
    ref = R.step64(*[sc[k] for k in KEYS], LAWS[law], DT, RADIUS, present=~gone, device=DEV)
    sc['position'] = sc['position'].copy()
    sc['position'][gone] = np.nan
    check_forward(f'skip_absent {name} {law}', forward(sc, law, skip_absent=True), ref, rows=~gone)
    assert np.isnan(forward(sc, law, skip_absent=False)).all()


@pytest.mark.parametrize('law', list(LAWS))
@pytest.mark.parametrize('name', ['clump200', 'clump2200'])
def test_fused_rollout_equals_operator_sequence_on_a_clump(name, law):
    from piml_amd.models.mlapm import MLAPM
    sc = R.case(name)
    gone = R.absent_mask(sc)
    args = [dev(sc[k]) for k in KEYS]
    args[0][dev(gone)] = float('nan')
    args[1][dev(gone)] = float('nan')
    m = MLAPM(version='UCY', **LAWS[law])
    fp, fv = m.rollout(*args, DT, RADIUS, steps=3)
    sp, sv = m.rollout(*args, DT, RADIUS, steps=3, fused=False)
    assert torch.equal(torch.isnan(fp), torch.isnan(sp)) and torch.equal(torch.isnan(fv), torch.isnan(sv))
    assert torch.equal(torch.isnan(fp[1, :, 0]).cpu(), torch.as_tensor(gone))          # frame 1 is a full step of the present agents
    assert torch.equal(torch.nan_to_num(fp), torch.nan_to_num(sp)) and torch.equal(torch.nan_to_num(fv), torch.nan_to_num(sv))


@pytest.mark.parametrize('name,entry', [('clump200', 'two_role'), ('clump700', 'ws')])
def test_operator_gradient_is_the_entry_point_tested_above(name, entry):
    """ops.mlapm_step's autograd picks the backward form by size: bitwise the direct call of that form"""
    from piml_amd import ops
    sc = R.case(name)
    w = dev(upstream(sc['position'].shape[0]))
    leaves = [dev(sc[k]).requires_grad_(True) for k in KEYS]
    act = ops.mlapm_step(*leaves, DT, RADIUS, version='UCY', **R.JUMP_LAW)
    got = torch.autograd.grad(act, leaves, w)
    rc, want = _mlapm_bwd_direct(entry, sc, w, 'UCY', law=R.JUMP_LAW)
    assert rc == 0
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy().reshape(r.shape), r)


def test_forward_and_both_backward_forms_are_bitwise_repeatable():
    sc = R.case('clump700')
    w = dev(upstream(700))
    for law in LAWS:
        a, b = forward(sc, law), forward(sc, law)
        assert np.array_equal(a, b)
        for entry in ('two_role', 'ws'):
            (rc0, g0), (rc1, g1) = [_mlapm_bwd_direct(entry, sc, w, 'UCY', law=LAWS[law]) for _ in range(2)]
            assert rc0 == 0 and rc1 == 0
            assert all(np.array_equal(x, y) for x, y in zip(g0, g1)), (law, entry)
