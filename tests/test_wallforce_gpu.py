"""GPU: the wall-force operator (piml_wall_force, ops_scenario.wall_force) against the numpy restatement (wallforce_ref.py):
index and dist2 bit for bit -- the brute force over every valid point against the kernel's 3 x 3 cell search --, the force
within 1e-5 relative of the float64 value (the bar mlapm.hpp states for the smooth law) with an absolute floor of 1e-6 Aw
for terms near the cutoff."""
import numpy as np
import pytest
import torch

import wallforce_ref as REF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32
CUTOFF, AW, BW = 2.0, 50.0, -5.0
FAR = (100.0, 100.0)                             # an isolated point on dyadic coordinates, 60 m from every other
ON_POINTS = 7


def special_rows():
    """a NaN position; an agent exactly on the isolated point (d2 == 0); exactly at d2 == c2 from it (not felt) and one
    float32 step inside (felt); outside the points' bounding box by less and by more than the cutoff"""
    inside = float(np.nextafter(f32(FAR[0] + CUTOFF), f32(0)))
    return np.array([[np.nan, 1.0], [1.0, np.nan], FAR, [FAR[0] + CUTOFF, FAR[1]], [inside, FAR[1]],
                     [FAR[0] + 1.0, FAR[1] + 1.0], [FAR[0] + 1.5, FAR[1] + 1.5], [300.0, -200.0], [-50.0, 20.0]], f32)


def make_case(rows, O, spread, invalid=0.0, seed=0):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(0, spread, (O, 2)).astype(f32)
    P = rng.uniform(-3, spread + 3, (rows, 2)).astype(f32)
    if invalid:
        bad = rng.random(O) < invalid
        obs[bad, rng.integers(0, 2, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum())).astype(f32)
    if O >= 7:
        obs[O // 2] = FAR
        sp = special_rows()
        P[:sp.shape[0]] = sp
        P[sp.shape[0]:sp.shape[0] + ON_POINTS] = obs[:ON_POINTS]       # agents exactly on points of the crowd of points too
    return P, obs


def square_case():
    from piml_amd.scenarios import four_directional_square_scenario
    obs = four_directional_square_scenario().obstacles.numpy()
    assert obs.shape == (128, 2)
    P = np.random.default_rng(9).uniform(-9, 9, (300, 2)).astype(f32)
    P[:16] = obs[::8]
    return P, obs


CASES = {'1x1': lambda: (np.array([[0.5, 0.25]], f32), np.array([[1.0, 1.0]], f32)),
         # two points equidistant on dyadic coordinates: the tie goes to the first in sorted order (one cell: list order)
         '1x2_tie': lambda: (np.array([[0.0, 0.0]], f32), np.array([[1.0, 0.5], [-1.0, 0.5]], f32)),
         '64x7': lambda: make_case(64, 7, 6.0, seed=1),
         # every point but the isolated one inside one cell: a run of 299 points, the lane stride loops five times
         '257x300_one_neighbourhood': lambda: make_case(257, 300, 1.5, seed=2),
         '300x4097': lambda: make_case(300, 4097, 40.0, seed=3),
         '200x900_30pct_invalid': lambda: make_case(200, 900, 25.0, invalid=0.3, seed=4),
         'square_128': square_case}


def run(P, obs, A=AW, B=BW, cutoff=CUTOFF):
    from piml_amd import ops_scenario
    g = ops_scenario.wall_grid(obs, cutoff, DEV)
    force, d2, idx = ops_scenario.wall_force(torch.from_numpy(P).to(DEV), g, A, B, return_selection=True)
    return g, force.cpu().numpy(), d2.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize('name', sorted(CASES))
def test_operator_against_the_restatement(name):
    P, obs = CASES[name]()
    g, force, d2, idx = run(P, obs)
    pts, order = REF.sorted_points(obs, CUTOFF)
    assert np.array_equal(g.host.points, pts) and np.array_equal(g.host.order, order)
    assert np.array_equal(g.points.cpu().numpy(), pts) and g.n_points == int(np.isfinite(obs).all(1).sum())
    want_i, want_d = REF.select(P, pts, CUTOFF)
    assert np.array_equal(idx, want_i), np.flatnonzero(idx != want_i)[:10]
    assert np.array_equal(d2.view(np.uint32), want_d.view(np.uint32))                  # bit for bit
    worst = REF.check_force(force, REF.force(P, pts, want_i, AW, BW), AW, name)
    felt = want_i >= 0
    print(f'\n[wallforce] {name}: {P.shape[0]} rows, {g.n_points} points, grid {g.gx} x {g.gy}, {int(felt.sum())} felt, '
          f'worst force error {worst:.3f} of the tolerance')
    assert (force[~felt] == 0).all()
    if name == '1x1':
        assert idx.tolist() == [0] and felt.all()
    if name == '1x2_tie':
        assert idx.tolist() == [0] and d2.tolist() == [1.25] and np.array_equal(pts[0], obs[0])
    if P.shape[0] >= 64 and name != 'square_128':
        n = special_rows().shape[0]
        far = int(np.flatnonzero((pts == f32(FAR)).all(1))[0])
        assert idx[:n].tolist() == [-1, -1, far, -1, far, far, -1, -1, -1]
        assert d2[2] == 0.0 and (force[2] == 0).all() and np.isinf(d2[3]) and d2[4] < f32(CUTOFF) * f32(CUTOFF)
        assert force[4, 0] > 0 and force[4, 1] == 0 and force[5, 0] > 0 and force[5, 1] > 0     # away from the wall
        on = slice(n, n + ON_POINTS)                             # on a point (an invalid one is a NaN position: not felt)
        assert (d2[on][felt[on]] == 0).all() and (force[on] == 0).all()
    if name == '257x300_one_neighbourhood':
        assert np.diff(g.host.cell_start).max() >= 299


@pytest.mark.parametrize('name', ['64x7', '300x4097', '200x900_30pct_invalid', '1x2_tie'])
def test_zero_strength_and_a_permutation_of_the_points(name):
    P, obs = CASES[name]()
    g, force, d2, idx = run(P, obs)
    _, zero, d2z, idxz = run(P, obs, A=0.0)
    assert (zero == 0).all() and np.array_equal(idx, idxz) and np.array_equal(d2.view(np.uint32), d2z.view(np.uint32))
    perm = np.random.default_rng(11).permutation(obs.shape[0])
    if name == '1x2_tie':
        perm = np.array([1, 0])
    gp, force_p, d2_p, idx_p = run(P, obs[perm])
    assert np.array_equal(d2.view(np.uint32), d2_p.view(np.uint32))                    # dist2 does not depend on the order
    assert np.array_equal(idx >= 0, idx_p >= 0)
    felt = np.flatnonzero(idx >= 0)
    a, b = g.host.points[idx[felt]], gp.host.points[idx_p[felt]]
    moved = felt[(a != b).any(1)]
    # the index changes only through the tie rule: another point at exactly the same float32 distance
    for i, qa, qb in zip(moved, a[(a != b).any(1)], b[(a != b).any(1)]):
        da = (qa - P[i]) * (qa - P[i])
        db = (qb - P[i]) * (qb - P[i])
        assert f32(da[0] + da[1]) == f32(db[0] + db[1]) == d2[i], (i, qa, qb)
    same = np.setdiff1d(felt, moved)
    assert np.array_equal(force[same].view(np.uint32), force_p[same].view(np.uint32))
    if name == '1x2_tie':
        assert moved.tolist() == [0] and idx_p.tolist() == [0] and np.array_equal(gp.host.points[0], obs[1])
    # the sorted index maps back to the obstacle list
    assert np.array_equal(obs[g.host.order[idx[felt]]], g.host.points[idx[felt]])


def test_leading_shapes_empty_problems_and_errors():
    from piml_amd import ops_scenario
    P, obs = CASES['300x4097']()
    g = ops_scenario.wall_grid(obs, CUTOFF, DEV)
    p = torch.from_numpy(P).to(DEV)
    flat, d2, idx = ops_scenario.wall_force(p, g, AW, BW, return_selection=True)
    f3, d3, i3 = ops_scenario.wall_force(p.reshape(3, 4, 25, 2), g, AW, BW, return_selection=True)
    assert f3.shape == (3, 4, 25, 2) and d3.shape == i3.shape == (3, 4, 25) and i3.dtype == torch.int32
    assert torch.equal(f3.reshape(-1, 2), flat) and torch.equal(i3.reshape(-1), idx) and torch.equal(d3.reshape(-1), d2)
    assert torch.equal(ops_scenario.wall_force(p, g, AW, BW), flat)
    half = ops_scenario.wall_force(p[::2], g, AW, BW)            # a strided view is made contiguous
    assert torch.equal(half, flat[::2])
    e, ed, ei = ops_scenario.wall_force(p[:0], g, AW, BW, return_selection=True)
    assert e.shape == (0, 2) and ed.shape == ei.shape == (0,)
    none = ops_scenario.wall_grid(np.full((5, 2), np.nan, f32), CUTOFF, DEV)             # no valid point: nothing is felt
    f0, d0, i0 = ops_scenario.wall_force(p, none, AW, BW, return_selection=True)
    assert none.n_points == 0 and (f0 == 0).all() and torch.isinf(d0).all() and (i0 == -1).all()
    with pytest.raises(ValueError):
        ops_scenario.wall_force(p, g, -1.0, BW)
    with pytest.raises(ValueError):
        ops_scenario.wall_force(p, g, AW, 0.5)
    with pytest.raises(ValueError):
        ops_scenario.wall_force(p.reshape(-1, 3), g, AW, BW)
    with pytest.raises(TypeError):
        ops_scenario.wall_force(p.double(), g, AW, BW)


def test_captured_replay_is_the_eager_call():
    from piml_amd import hip_graphs_safe, ops_scenario
    assert hip_graphs_safe()
    P, obs = CASES['300x4097']()
    g = ops_scenario.wall_grid(obs, CUTOFF, DEV)
    p = torch.from_numpy(P).to(DEV)
    eager = ops_scenario.wall_force(p, g, AW, BW)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops_scenario.wall_force(p, g, AW, BW)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
