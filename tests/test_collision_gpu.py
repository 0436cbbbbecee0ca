"""The collision predicates of csrc/pairwise.hip at their edges: a threshold met within an ulp, the friends rule's 25 / 26
boundary, and the shapes at which ops.collision_counts changes kernel.  Every count is an integer and every comparison is
exact, against the oracle's collision_detection (or collision_ref.counts_ref where the (S, N, N) matrices would not fit).

Kernels and template arities launched (T = number of thresholds, W = waves per workgroup):
  threshold boundary   collision_counts_fast_kernel<4, T> (S = 3) and <16, T> (S = 12), collision_counts_frames_kernel<4, T>
                       and <16, T>, collision_grid_kernel<T, 0 / 1>, collision_totals_kernel<T> with
                       collision_counts_from_totals_kernel<T>, collision_counts_kernel<4>, collision_pairs4_kernel with
                       collision_friends3_kernel -- each for T = 1, 2 and 4
  friends boundary     the grid, two-sweep (T = 2) and scratch-free (<4>, 2 and 5 thresholds) forms, collision_pairs_kernel /
                       collision_pairs4_kernel with collision_friends3_kernel (with and without real_position),
                       collision_counts_fast_kernel<4, 2> at S = 25
  beyond 4096 slices   collision_counts_kernel<1>
  grid edges           collision_grid_kernel<1 / 2, .> and the two-sweep kernels <1 / 2>, N = 5800 with more than 64 KiB of LDS
  matrices             collision_pairs_kernel, collision_pairs4_kernel, collision_friends4_kernel
  label                collision_label_kernel
"""
import numpy as np
import pytest
import torch

from collision_ref import F32, counts_ref, friends_boundary_scene, lattice_scene, near_threshold_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEAR_SLICES = 27
NEAR_SEEDS = {0.5: 0, 0.25: 1, 0.3: 2, 0.15: 3, 1 / 3: 4, 7.3: 5, 1e-3: 6}


def dev(x):
    return torch.from_numpy(np.array(x, order='C')).to(DEV)          # a copy: the cached scenes are read-only


def raw_counts(p, thr):
    """piml_collision_counts itself: above 25 slices the scratch-free collision_counts_kernel, whatever the number of thresholds."""
    from piml_amd import _lib
    S, N = p.shape[0], p.shape[1]
    t = torch.tensor([float(x) for x in thr], device=DEV, dtype=torch.float32)
    out = torch.full((len(thr), S, N), -1.0, device=DEV)
    _lib.check(_lib.lib().piml_collision_counts(p.data_ptr(), S, N, t.data_ptr(), len(thr), out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), 'piml_collision_counts')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_counts(oracle, p, thr):
    return np.stack([oracle.collision_detection(p, t).sum(-1) for t in thr])


def many_slice_forms(ops, monkeypatch, p, thr):
    """The three forms behind more than 25 slices (at most 4 thresholds): name -> counts."""
    out = {}
    for grid in (True, False):
        monkeypatch.setattr(ops, 'COLLISION_GRID', grid)
        out['grid' if grid else 'two-sweep'] = ops.collision_counts(p, thr).cpu().numpy()
    monkeypatch.setattr(ops, 'COLLISION_GRID', True)
    out['scratch-free'] = raw_counts(p, thr)
    return out


def matrix_counts(ops, p, thr):
    return np.stack([ops.collision_detection(p, t).sum(-1).cpu().numpy() for t in thr])


# ---- a threshold met within an ulp ----

@pytest.mark.parametrize('thr', [(0.5, 0.25), (0.3, 0.15), (1 / 3,), (7.3, 1e-3, 0.3, 0.5)], ids=lambda t: 'x'.join(f'{x:.3g}' for x in t))
def test_threshold_boundary_all_forms(oracle, monkeypatch, thr):
    """Pairs within 4 ulp of a threshold (256 of them a slice, a scene for each threshold of the tuple, counted at the whole
    tuple) through every counting form.  A cut of sq_below or lt_cut2 that is one float off, or thr * thr in its place, flips
    some of these pairs (test_collision_ref.py shows it for each threshold)."""
    from piml_amd import ops
    for scene_thr in thr:
        pn = near_threshold_scene(scene_thr, 256, NEAR_SLICES, NEAR_SEEDS[scene_thr])
        p = dev(pn)
        N = pn.shape[1]
        each = oracle_counts(oracle, pn[:25], thr)                   # at most 25 slices: every slice on its own
        assert 0 < each[thr.index(scene_thr)].sum() < 25 * N
        # fast form: 4 waves (S N < 4096) and 16 waves
        for S in (3, 12):
            got = ops.collision_counts(p[:S], thr).cpu().numpy()
            assert np.array_equal(got, each[:, :S]), ('fast', scene_thr, S, np.abs(got - each[:, :S]).sum())
        # frames variant: 5 frames of 1 slice (4 waves) and of 3 slices (16 waves)
        for S in (1, 3):
            recs = ops.collision_counts_frames([p[f * S:(f + 1) * S] for f in range(5)], thr)
            assert len(recs) == 5
            for f, rec in enumerate(recs):
                assert np.array_equal(rec.cpu().numpy(), each[:, f * S:(f + 1) * S]), ('frames', scene_thr, S, f)
        # 27 slices: the grid, the two sweeps, the scratch-free kernel, the matrices
        want = oracle_counts(oracle, pn, thr)
        for name, got in many_slice_forms(ops, monkeypatch, p, thr).items():
            assert np.array_equal(got, want), (name, scene_thr, np.abs(got - want).sum())
        assert np.array_equal(matrix_counts(ops, p, thr), want), ('matrix', scene_thr)


# ---- the friends rule: kept up to 25 slices, dropped from 26 ----

FRIENDS_THR = (0.5, 0.25)


@pytest.mark.parametrize('S', [26, 33, 65])
def test_friends_boundary_all_forms(oracle, monkeypatch, S):
    """Pairs colliding in exactly 24, 25, 26 and 27 slices (with 33 and 65 slices their totals come from two chunks of the
    two-sweep form), a pair with 26 at the high and 25 at the low threshold, one that reaches 25 through absences, one that
    collides throughout.  t < 25, t <= 26 or the other threshold's totals in any one form change a count here."""
    from piml_amd import ops
    pn, pairs = friends_boundary_scene(S, FRIENDS_THR, 3)
    p = dev(pn)
    want = oracle_counts(oracle, pn, FRIENDS_THR)
    for name, (i, j, hi, lo) in pairs.items():                      # what the scene is for, in the reference's own counts
        for h, tot in enumerate((hi, lo)):
            kept = tot if tot <= 25 else 0
            assert want[h, :, i].sum() == kept == want[h, :, j].sum(), (name, h)
    assert pairs['c25'][2] == 25 and pairs['c26'][2] == 26 and pairs['split'][2:] == (26, 25)
    for name, got in many_slice_forms(ops, monkeypatch, p, FRIENDS_THR).items():
        assert np.array_equal(got, want), (name, S, np.argwhere(got != want)[:8])
    five = FRIENDS_THR + (0.3, 1.0, 0.05)                             # 5 thresholds: ops reaches the scratch-free kernel
    got = ops.collision_counts(p, five).cpu().numpy()
    assert np.array_equal(got, oracle_counts(oracle, pn, five)), ('five thresholds', S)
    assert np.array_equal(matrix_counts(ops, p, FRIENDS_THR), want), ('matrix', S)


@pytest.mark.parametrize('S', [26, 33])
def test_friends_boundary_on_real_position(oracle, S):
    """With real_position the 25 / 26 boundary is taken on ITS collisions: the counted positions have every designated pair
    together in all slices, and the pairs that the base keeps are the ones with at most 25."""
    from piml_amd import ops
    base, pairs = friends_boundary_scene(S, FRIENDS_THR, 3)
    q = base.copy()
    for i, j, _, _ in pairs.values():
        q[:, j] = q[:, i] + F32(0.1)
    for h, t in enumerate(FRIENDS_THR):
        want = oracle.collision_detection(q, t, real_position=base)
        got = ops.collision_detection(dev(q), t, real_position=dev(base)).cpu().numpy()
        assert np.array_equal(got, want), (S, t)
        for name, (i, j, *tot) in pairs.items():
            if name != 'absent':                                     # (its counted copy is absent in some slices too)
                assert want[:, i, j].sum() == (S if tot[h] <= 25 else 0), (name, t)


def test_friends_rule_idle_at_25_slices(oracle):
    """25 slices: a pair that collides in every one of them is kept, by the fast form and by the matrix form."""
    from piml_amd import ops
    pn, pairs = friends_boundary_scene(25, FRIENDS_THR, 3)
    i, j, hi, lo = pairs['always']
    assert (hi, lo) == (25, 25)
    want = oracle_counts(oracle, pn, FRIENDS_THR)
    assert want[0, :, i].sum() == 25 == want[1, :, j].sum()
    assert np.array_equal(ops.collision_counts(dev(pn), FRIENDS_THR).cpu().numpy(), want)
    assert np.array_equal(matrix_counts(ops, dev(pn), FRIENDS_THR), want)


def test_scratch_free_kernel_beyond_4096_slices(oracle):
    """4097 slices with 5 thresholds: one agent per workgroup with its per-slice counters in LDS above 16 KiB
    (collision_counts_kernel<1>), with a pair together in 26 slices (dropped) and one in 25 (kept), the last slice among them."""
    from piml_amd import ops
    S, N = 4097, 6
    rng = np.random.default_rng(9)
    pn = (np.arange(N)[None, :, None] * 10.0 + rng.random((S, N, 2))).astype(F32)     # 10 m apart: nobody collides
    s26 = np.r_[rng.choice(S - 1, 25, replace=False), S - 1]
    s25 = np.r_[rng.choice(S - 1, 24, replace=False), S - 1]
    pn[s26, 1] = pn[s26, 0] + F32(0.1)
    pn[s25, 3] = pn[s25, 2] + F32(0.1)
    pn[5::7, 5] = np.nan
    thr = (0.5, 0.25, 0.3, 1.0, 0.05)
    want = oracle_counts(oracle, pn, thr)
    assert want[0, :, 0].sum() == 0 and want[0, :, 2].sum() == 25 and want[4].sum() == 0
    got = ops.collision_counts(dev(pn), thr).cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# ---- the cell grid's edges ----

def both_sweeps(ops, monkeypatch, p, thr):
    out = {}
    for grid in (True, False):
        monkeypatch.setattr(ops, 'COLLISION_GRID', grid)
        out['grid' if grid else 'two-sweep'] = ops.collision_counts(p, thr).cpu().numpy()
    return out


def test_grid_with_more_than_64k_of_lds(monkeypatch):
    """5800 agents: the sorted positions and indices take 58 000 bytes on top of the 8 KiB of cell counters."""
    from piml_amd import ops
    pn = lattice_scene(26, 5800, 40, 21)
    want = counts_ref(pn, 0.5)
    assert want.sum() > 5800 and (want == 0).any()
    for name, got in both_sweeps(ops, monkeypatch, dev(pn), (0.5,)).items():
        assert got.shape == (1, 26, 5800)
        assert np.array_equal(got[0], want), (name, np.argwhere(got[0] != want)[:8])


def grid_edge_scene():
    """26 slices of 300 agents on the lattice: slices 0 .. 5 with every agent inside one 0.51 m cell ([0, 0.5]^2), the others
    spread over 60 m in both axes (more than 32 cells: the torus aliases), negative coordinates, absent agents; agents 0 .. 3
    in the torus' last cell (31, 31) = index 1023 from slice 6 on, agents 4 and 5 next to them in the cells that wrap to
    column 0 and row 0."""
    rng = np.random.default_rng(31)
    p = lattice_scene(26, 300, 30, 32)
    p[:6] = (rng.integers(0, 3, size=(6, 300, 2)) * 0.25).astype(F32)
    p[:6][rng.random((6, 300)) < 0.05] = np.nan
    p[6:, 0] = (16.0, 16.0)
    p[6:, 1] = (16.25, 16.0)
    p[6:20, 2] = (16.0, 16.25)
    p[6:, 3] = (16.25, 16.25)
    p[6:, 4] = (16.5, 16.0)
    p[6:, 5] = (16.25, 16.5)
    c = float(F32(0.5) * F32(1.02))
    assert np.floor(p[6, :4] / c).astype(int).tolist() == [[31, 31]] * 4 and np.floor(16.5 / c) == 32
    assert np.ptp(np.floor(p[7, 6:, 0][~np.isnan(p[7, 6:, 0])] / c)) > 32 and np.nanmax(p[:6]) < c
    return p


def test_grid_one_cell_last_cell_and_aliases(oracle, monkeypatch):
    from piml_amd import ops
    pn = grid_edge_scene()
    thr = (0.5, 0.25)
    want = oracle_counts(oracle, pn, thr)
    assert np.median(want[0, 0]) > 30 and want[0, 6:, 0].sum() > 0        # a crowded cell; the last cell's agents collide
    for name, got in both_sweeps(ops, monkeypatch, dev(pn), thr).items():
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8])


@pytest.mark.parametrize('thr', [(0.0, 0.5), (-1.0,)], ids=['0x0.5', '-1'])
def test_degenerate_thresholds(oracle, monkeypatch, thr):
    """A threshold of zero keeps the square root for the whole tuple; a negative one alone gives a cell size of zero, so
    every frame walks all pairs.  No pair is closer than a non-positive threshold -- and neither is an agent to itself, so
    the identity that collision_detection subtracts whatever the threshold (data.py:562) leaves -1 for every present agent
    and 0 for an absent one: that is what the reference's .sum(-1) holds, and what the counting forms have to give."""
    from piml_amd import ops
    pn = grid_edge_scene()
    want = oracle_counts(oracle, pn, thr)
    present = (~np.isnan(pn).any(-1)).astype(np.float32)
    for h, t in enumerate(thr):
        assert t > 0 or np.array_equal(want[h], -present)              # no pair collides; the agent's own entry is 0 - 1
    for name, got in both_sweeps(ops, monkeypatch, dev(pn), thr).items():
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8])
    p25 = dev(pn[:25])                                                   # the fast form, the scratch-free kernel, the matrices
    assert np.array_equal(ops.collision_counts(p25, thr).cpu().numpy(), oracle_counts(oracle, pn[:25], thr))
    assert np.array_equal(raw_counts(dev(pn), thr), want)
    assert np.array_equal(matrix_counts(ops, dev(pn), thr), want)


# ---- the matrix kernels ----

@pytest.mark.parametrize('N', [12, 1028, 1032, 257, 1027])
@pytest.mark.parametrize('S', [1, 3])
def test_collision_matrix_shapes(oracle, S, N):
    """N % 4 == 0 takes the float4 kernel (12: a row block of 4; 1028 and 1032: two x-blocks, 1028 with a row tail), the
    others the scalar one with several x-blocks; distances exactly on the threshold, absent agents, with and without - I."""
    from piml_amd import ops
    pn = lattice_scene(S, N, 1 if N < 100 else 5, 100 + N)
    pn[:, :4] = np.array([[0.5, -0.25], [0.5, -0.25], [-1.0, 1.0], [-0.75, 1.0]], F32)     # at one point; exactly 0.25 m apart
    valid = ~np.isnan(pn).any(-1)
    for thr in (0.5, 0.25):
        want = oracle.collision_detection(pn, thr)                  # at most 25 slices: the pairs minus the identity
        assert want.sum() > 0
        got = ops.collision_matrix(dev(pn), thr, True).cpu().numpy()
        assert np.array_equal(got, want), (thr, np.argwhere(got != want)[:8])
        plain = want + np.eye(N, dtype=np.float32) * valid[:, :, None]
        got = ops.collision_matrix(dev(pn), thr, False).cpu().numpy()
        assert np.array_equal(got, plain), (thr, np.argwhere(got != plain)[:8])


@pytest.mark.parametrize('N', [37, 40])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 5])
def test_friends_rule_4d_first_four_frames(oracle, T, N):
    """(C, T, N, 2): a pair that collides in any of the first min(T, 4) frames of a channel is dropped in all of its frames.
    Pair (0, 1) collides in frame 3 only (dropped wherever it exists), pair (2, 3) in frame 4 only (kept), pair (4, 5) in
    every frame (dropped in every frame, whatever T)."""
    from piml_amd import ops
    C = 3
    pn = lattice_scene(C * T, N, 4, 200 + T, nan_frac=0.1).reshape(C, T, N, 2)
    pn[:, :, :6] = np.array([[-50.0, 0.0], [-40.0, 0.0], [-30.0, 0.0], [-20.0, 0.0], [-10.0, 0.0], [-10.0, 0.25]], F32)
    if T > 3:
        pn[:, 3, 1] = pn[:, 3, 0] + F32(0.25)
    if T > 4:
        pn[:, 4, 3] = pn[:, 4, 2] + F32(0.25)
    for thr in (0.5, 1.0):
        want = oracle.collision_detection(pn, thr)
        got = ops.collision_detection(dev(pn), thr).cpu().numpy()
        assert got.shape == (C, T, N, N)
        assert np.array_equal(got, want), (thr, np.argwhere(got != want)[:8])
        assert want[:, :, 0, 1].sum() == 0 and want[:, :, 4, 5].sum() == 0
        assert T < 5 or (want[:, 4, 2, 3] == 1).all() and want[:, :4, 2, 3].sum() == 0
        assert T < 5 or want[:, 4].sum() > 0


# ---- the one-second collision label ----

def label_rows(stride):
    """Rows (dp, dv, ...) of `stride` columns: 4096 random ones, |dp| within 4 ulp of 0.5 with dv = 0, dp = 0 with and
    without dv, and rows with a NaN in each of the four columns."""
    rng = np.random.default_rng(40 + stride)
    rnd = rng.normal(size=(4096, stride)).astype(F32)
    rnd[:, :2] *= F32(0.8)
    near = np.zeros((512, stride), F32)
    r = np.float64(F32(0.5)) * (1.0 + rng.integers(-4, 5, size=512) * 2.0 ** -24)
    ang = rng.random(512) * 2 * np.pi
    ang[:128] = np.repeat([0.0, np.pi / 2, np.pi, 3 * np.pi / 2], 32)                  # on the axes the norm is |x| itself
    near[:, 0], near[:, 1] = r * np.cos(ang), r * np.sin(ang)
    near[np.abs(near) < 1e-12] = 0
    near[:, 4:] = rng.normal(size=(512, stride - 4))
    zero = np.zeros((64, stride), F32)
    zero[32:, 2:4] = rng.normal(size=(32, 2))
    zero[32, 2:4] = (1e-3, 0.0)                                                          # barely moving
    nan = rng.normal(size=(64, stride)).astype(F32) * F32(0.3)
    nan[np.arange(64), np.arange(64) % 4] = np.nan
    return rnd, near, zero, nan


@pytest.mark.parametrize('stride', [4, 6])
def test_collision_label_edges(oracle, stride):
    from piml_amd import ops
    rnd, near, zero, nan = label_rows(stride)
    for name, rows in (('random', rnd), ('near 0.5', near), ('dp = 0', zero), ('nan', nan)):
        want = oracle.collision_label(rows)
        got = ops.collision_label(dev(rows)).cpu().numpy()
        assert got.shape == rows.shape[:-1]
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8])
        if name in ('random', 'near 0.5'):
            assert 0.1 < want.mean() < 0.9, (name, want.mean())      # both labels occur
    want = oracle.collision_label(zero)
    assert (want[:32] == 0).all() and (want[32:] == 1).all()         # dp = 0: no label at rest, a label once it moves
    batched = ops.collision_label(dev(rnd.reshape(8, 64, 8, stride))).cpu().numpy()
    assert np.array_equal(batched, oracle.collision_label(rnd).reshape(8, 64, 8))
