"""The scenes of collision_ref.py do what the GPU tests of test_collision_gpu.py rely on (no GPU needed): the
near-threshold pairs straddle the threshold and hit it exactly, a squared-domain cut that is one float off flips some of
them, the friends-boundary pairs have exactly the totals they are named after, and counts_ref equals the oracle."""
import numpy as np
import pytest

from collision_ref import (F32, counts_ref, d2_f32, dist_f32, friends_boundary_scene, lattice_scene, near_threshold_scene,
                           sq_cut)

THRESHOLDS = (0.5, 0.25, 0.3, 0.15, 1 / 3, 7.3, 1e-3)
NPAIRS, SLICES = 256, 3


@pytest.mark.parametrize('thr', THRESHOLDS)
def test_near_threshold_scene_straddles_and_hits_the_threshold(oracle, thr):
    p = near_threshold_scene(thr, NPAIRS, SLICES, THRESHOLDS.index(thr))
    assert p.shape == (SLICES, 2 * NPAIRS, 2) and p.dtype == np.float32
    coll = oracle.collision_detection(p, thr)                            # 3 slices: the friends rule cannot fire
    m = np.arange(NPAIRS)
    pair = coll[:, 2 * m, 2 * m + 1]
    assert np.array_equal(pair, coll[:, 2 * m + 1, 2 * m])
    frac = pair.mean()
    d = dist_f32(p[:, 0::2], p[:, 1::2])
    exact = (d == F32(thr)).mean()
    print(f'thr {thr}: colliding {frac:.3f}, exactly on the threshold {exact:.3f}')
    assert 0.2 <= frac <= 0.8
    assert exact >= 0.05
    assert coll.sum() == 2 * pair.sum()                                  # nothing but the designated pairs collides
    assert np.array_equal(pair, (d < F32(thr)).astype(np.float32))       # the numpy restatement is the oracle's predicate


@pytest.mark.parametrize('thr', THRESHOLDS)
def test_near_threshold_scene_feels_a_cut_one_float_off(oracle, thr):
    p = near_threshold_scene(thr, NPAIRS, SLICES, THRESHOLDS.index(thr))
    m = np.arange(NPAIRS)
    want = oracle.collision_detection(p, thr)[:, 2 * m, 2 * m + 1] > 0
    d2 = d2_f32(p[:, 0::2], p[:, 1::2])
    cut = sq_cut(thr)
    assert np.sqrt(cut, dtype=F32) < F32(thr) <= np.sqrt(np.nextafter(cut, F32(np.inf)), dtype=F32)
    assert np.array_equal(d2 <= cut, want)                               # the squared-domain test with the searched cut
    up = int(((d2 <= np.nextafter(cut, F32(np.inf))) != want).sum())
    down = int(((d2 <= np.nextafter(cut, F32(-np.inf))) != want).sum())
    naive = int(((d2 < F32(thr) * F32(thr)) != want).sum())
    print(f'thr {thr}: flipped by cut + 1 ulp {up}, by cut - 1 ulp {down}, by the naive thr * thr {naive}')
    assert up >= 1 and down >= 1


@pytest.mark.parametrize('S', [25, 26, 33, 65])
def test_friends_boundary_scene_totals(oracle, S):
    thr = (0.5, 0.25)
    p, pairs = friends_boundary_scene(S, thr, 3)
    assert set(pairs) == {'c24', 'c25', 'c26', 'c27', 'split', 'absent', 'always'}
    if S >= 27:
        assert [pairs[n][2] for n in ('c24', 'c25', 'c26', 'c27')] == [24, 25, 26, 27]
    for h, t in enumerate(thr):
        raw = np.stack([oracle.collision_detection(p[s:s + 1], t)[0] for s in range(S)])      # slice by slice: no rule
        kept = oracle.collision_detection(p, t)
        designated = np.zeros(raw.shape[1:], bool)
        for name, (i, j, *tot) in pairs.items():
            designated[i, j] = designated[j, i] = True
            assert raw[:, i, j].sum() == tot[h] == raw[:, j, i].sum(), (name, t)
            want = raw[:, i, j] if tot[h] <= 25 else np.zeros(S, np.float32)
            assert np.array_equal(kept[:, i, j], want) and np.array_equal(kept[:, j, i], want), (name, t)
        assert raw[:, ~designated].sum() == 0                                     # the background never collides
        assert kept.sum() == 2 * sum(v[2 + h] for v in pairs.values() if v[2 + h] <= 25)
    if S >= 26:
        assert pairs['split'][2:] == (26, 25) and pairs['absent'][2:] == (25, 25) and pairs['always'][2:] == (S, S)


def test_counts_ref_equals_oracle_on_a_lattice(oracle):
    p = lattice_scene(40, 200, 6, 7, nan_frac=0.08)
    assert np.nanmin(p) < 0 < np.nanmax(p) and np.array_equal(p[~np.isnan(p)] * 4, np.round(p[~np.isnan(p)] * 4))
    for thr in (0.25, 0.5, 1.0):
        want = oracle.collision_detection(p, thr).sum(-1)
        raw = sum(oracle.collision_detection(p[s:s + 1], thr).sum() for s in range(40))
        assert 0 < want.sum() <= raw
        assert thr < 0.5 or want.sum() < raw                             # from 0.5 m on there are friends the rule removes
        assert np.array_equal(counts_ref(p, thr), want), thr
