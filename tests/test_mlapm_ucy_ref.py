"""CPU: the float64 UCY yardstick of tests/mlapm_ucy_ref.py against the reference's committed goldens, and the conditions
the scenes of tests/test_mlapm_ucy_gpu.py exist for -- every pair decidable, the rings filled -- asserted from the float64
filter, not from a kernel."""
import numpy as np
import pytest

import mlapm_ucy_ref as R
from conftest import golden

RADIUS = 0.3


@pytest.mark.parametrize('N', [7, 64, 1024])
def test_step64_matches_the_reference_goldens(N):
    """The project's own bars for the kernel (1e-5 relative, floor 1e-3; gradients 2e-5 of the largest entry) hold for the
    yardstick with room: measured 8.3e-7 (action) and 3.6e-7 (gradients) at worst, against the reference's float32 numbers."""
    g = golden('mlapm')
    k = f'UCY_N{N}'
    tau, A, B, C, _, theta = [float(x) for x in g['UCY_params']]
    s = R.step64(g[k + '_p'], g[k + '_v'], g[k + '_v0'], g[k + '_dest'], dict(tau=tau, A=A, B=B, C=C, theta=theta), 0.08,
                 RADIUS, w=g[k + '_w'])
    ref = g[k + '_action']
    err = (np.linalg.norm(s.action - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-3)).max()
    assert err < 1e-5, err
    for got, name in zip(s.grads, ('gp', 'gv', 'gv0', 'gdest')):
        ref = g[f'{k}_{name}']
        d = np.abs(got.reshape(ref.shape) - ref).max()
        assert d <= 2e-5 * max(np.abs(ref).max(), 1e-3), (name, d)
    assert (s.m >= np.linalg.norm(s.action, axis=-1) * (1 - 1e-12)).all()        # m bounds the output it is made of


def test_step64_with_absent_agents_is_the_compacted_scene():
    sc = R.case('clump130')
    gone = R.absent_mask(sc)
    args = [sc[k] for k in ('position', 'velocity', 'desired_speed', 'destination')]
    full = R.step64(*args, R.UCY_LAW, 0.08, RADIUS, present=~gone)
    sub = R.step64(*[a[~gone] for a in args], R.UCY_LAW, 0.08, RADIUS)
    assert np.array_equal(full.action[~gone], sub.action) and np.isnan(full.action[gone]).all()
    assert np.array_equal(full.m[~gone], sub.m)


def _present_variants(sc):
    """the scene as the forward / backward tests see it, and as the skip_absent and rollout tests do (compacted)"""
    gone = R.absent_mask(sc)
    yield 'all', sc['position'], sc['velocity'], sc['destination']
    yield 'present', sc['position'][~gone], sc['velocity'][~gone], sc['destination'][~gone]


@pytest.mark.parametrize('name', R.CASES)
def test_every_pair_of_every_scene_is_decidable(name):
    """A condition on the inputs, not a tolerance: no off-diagonal pair's flag depends on float32 against float64 or on
    thresholds moved by DELTA = 1e-4, and no pair is within KINK of a view or rotation-sign crossing."""
    sc = R.case(name)
    for tag, p, v, dest in _present_variants(sc):
        flag, decidable = R.flags(p, v, RADIUS)
        assert flag.shape == (len(p), len(p)) and np.array_equal(flag, flag.T)
        assert int((~decidable).sum()) == 0, (name, tag, np.argwhere(~decidable)[:5])
        assert R.kink_margin(p, v, dest) >= R.KINK, (name, tag)
        cand = R.candidates(p, v, RADIUS)
        assert not (flag & ~cand).any(), (name, tag)             # the float64 filter is conservative on these scenes


@pytest.mark.parametrize('name', list(R.CLUMP_SHAPES))
def test_clump_scenes_fill_the_rings(name):
    N, lo, n = R.CLUMP_SHAPES[name]
    sc = R.case(name)
    clump = sc['clump']
    assert clump.sum() == n and clump[lo] and clump[lo + n - 1] and sc['position'].shape == (N, 2)
    p, v = sc['position'], sc['velocity']
    d = np.linalg.norm(p[clump].astype(np.float64)[None] - p[clump].astype(np.float64)[:, None], axis=-1)
    assert d.max() < 0.54 and d[~np.eye(n, dtype=bool)].min() >= 0.02 * (1 - 1e-6)
    flag = R.flags(p, v, RADIUS)[0]
    cand = R.candidates(p, v, RADIUS)
    assert flag[np.ix_(clump, clump)].all() and cand[np.ix_(clump, clump)].all()     # every clump pair: candidate and flagged
    per_tile = np.stack([cand[clump][:, b:b + R.TILE].sum(1) for b in range(0, N, R.TILE)], axis=1)
    if lo + n <= R.TILE:
        # >= 128 candidates of every clump agent inside one tile: the 128-entry backward ring wraps (its indices run on through
        # a tile) and at least two mid-tile drains follow each other; the forward's 256-entry ring wraps from 257 on
        assert (per_tile.max(1) >= 128).all(), per_tile.max(1).min()
        if name == 'clump310':
            assert (per_tile.max(1) >= 257).all(), per_tile.max(1).min()
    else:
        # the clump straddles index 2048: its 200 agents are 98 + 102, so no tile can hold 128 of them; what this shape is
        # for is a ring that drains mid-tile and again at the end of BOTH tiles
        assert per_tile.shape[1] == 2 and clump[:R.TILE].sum() == 98 and clump[R.TILE:].sum() == 102
        assert (per_tile >= 64).all(), per_tile.min(0)
    # a full 64-of-64 batch: some aligned block of 64 sources lies inside the clump
    assert any(clump[b:b + 64].all() for b in range(0, N - 63, 64))
    if name == 'clump700':
        assert lo % 64 and (lo + n) % 64 and lo % 128 and (lo + n) % 128         # not aligned to a batch
    # with a tenth of the agents absent the clump still fills a 64-batch ring more than once
    gone = R.absent_mask(sc)
    assert gone[0] and gone[-1] and (gone & clump).any() and abs(int(gone.sum()) - N // 10) <= 1
    assert (gone & ~clump).any() or clump.all()
    assert (cand[np.ix_(clump & ~gone, ~gone)].sum(1) >= 90).all()


def test_boundary_scene_pairs_are_what_their_construction_says():
    two_r = float(np.float32(RADIUS) * np.float32(2))
    for name in ('boundary', 'boundary_apart'):
        sc = R.case(name)
        p, v = sc['position'].astype(np.float64), sc['velocity'].astype(np.float64)
        flag = R.flags(sc['position'], sc['velocity'], RADIUS)[0]
        cand = R.candidates(sc['position'], sc['velocity'], RADIUS)
        kinds = set()
        built = np.zeros_like(flag)
        for i, j, kind, expect in sc['pairs']:
            kinds.add(kind)
            built[i, j] = built[j, i] = True
            assert flag[i, j] == expect and flag[j, i] == expect, (name, i, j, kind, expect)
            r, w = p[j] - p[i], v[j] - v[i]
            a = np.linalg.norm(r) - np.linalg.norm(w)
            if kind == 'head-on':
                # the float32 arrays realise |r| - |w| = 2R (1 -+ 1e-3) to a fifth of the margin, and w is antiparallel to r
                assert abs(abs(a / two_r - 1) - 1e-3) < 2e-4 and (a < two_r) == expect, (i, j, a)
                assert abs(np.linalg.norm(r + w) - a) < 1e-6 * np.linalg.norm(r)
            if kind == 'glancing':
                t = -(r @ w) / (w @ w)
                dmin = np.sqrt(r @ r - (r @ w) ** 2 / (w @ w))
                assert min(abs(t - x) for x in (0.05, 0.5, 0.95)) < 1e-4, (i, j, t)
                assert abs(abs(dmin / two_r - 1) - 1e-3) < 2e-4 and (dmin < two_r) == expect, (i, j, dmin)
                assert np.linalg.norm(r) > two_r * 2 and np.linalg.norm(r + w) > two_r * (1 + 1e-3)   # the third clause alone
            if kind in ('rest', 'together'):
                assert (w == 0).all()
            if kind == 'coincident':
                assert ((r == 0).all() and (w != 0).any()) if name == 'boundary' else np.linalg.norm(r) > 0.29
            assert cand[i, j] and cand[j, i] or not expect
        assert kinds == {'head-on', 'glancing', 'rest', 'together', 'coincident'}
        np.fill_diagonal(built, True)
        assert not flag[~built].any() and not cand[~built].any()      # pairs of different constructions: far, by the filter too
        # the outside pairs at short range are what the filter may call far; at long range its slack keeps them candidates
        far_outside = [(i, j) for i, j, kind, e in sc['pairs'] if not e and not cand[i, j]]
        near_outside = [(i, j) for i, j, kind, e in sc['pairs'] if not e and cand[i, j]]
        assert far_outside and near_outside


def test_sparse_scene_has_no_candidates():
    for name in ('sparse257', 'sparse257_drift'):
        sc = R.case(name)
        cand = R.candidates(sc['position'], sc['velocity'], RADIUS)
        assert int(cand.sum()) == 257                             # the diagonal only
        assert not R.flags(sc['position'], sc['velocity'], RADIUS)[0][~np.eye(257, dtype=bool)].any()
    assert (R.case('sparse257')['velocity'] == 0).all()


def test_float32_restatement_is_within_the_bars():
    """What the issue asks to check before a bar is called unreachable on a scene: the same law in float32 torch against
    step64, in the forward test's measure |err_i| / max(m_i, 1e-3) (bar 1e-5)."""
    for name in ('clump130', 'clump200', 'boundary'):
        sc = R.case(name)
        args = [sc[k] for k in ('position', 'velocity', 'desired_speed', 'destination')]
        for law in (R.UCY_LAW, R.JUMP_LAW):
            ref = R.step64(*args, law, 0.08, RADIUS)
            got = R.step32(*args, law, 0.08, RADIUS)
            ratio = (np.linalg.norm(got - ref.action, axis=-1) / np.maximum(ref.m, 1e-3)).max()
            print(f'{name} float32 torch vs float64: worst |err| / m = {ratio:.2e}')
            assert ratio < 1e-5 / 4, (name, ratio)
