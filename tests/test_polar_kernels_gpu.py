"""The two hand-written kernels under `--model pinnsf_pb` / `pinnsf_pbc` away from the captured scenes:

1. the collision post-correction (piml_amd/csrc/pairwise.hip, ops.collision_post_correction) against a float64 evaluation of
   `torch_correction` (tests/test_polar_gpu.py), branch by branch, on seeded random neighbourhoods, plus hand-built edges;
2. the temporal heading fill (piml_amd/csrc/relfeat.hip, ops.heading_direction) bit for bit against a numpy restatement of
   Pedestrians.get_heading_direction (src/data/data.py:350-395), which a CPU test pins on the `relfeat_*` golden arrays;
3. both polar models against a float64 evaluation of the same weights.

The correction makes discrete choices (inside the radius, head-on or chasing, nearest of a kind, s > 0, q < 0).  A float32
evaluation may fall on the other side of a choice than float64 when a row is within rounding of it, so every comparison with
float64 is restricted to the rows whose decision margins -- computed from the float64 evaluation alone -- are at least 1e-4."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from conftest import bits, golden, golden_names
from test_polar_gpu import load, torch_correction

gpu = pytest.mark.gpu
DEV = 'cuda'
THR, DT = 0.5, 0.08
MARGIN, NEAR = 1e-4, 1e-2


# ------------------------------------------------------------------------------------------------
# 1. collision post-correction
# ------------------------------------------------------------------------------------------------
def neighbourhoods(lead, k, stride, seed):
    """(predictions, ped_features, velocity, upstream gradient), float32 on the CPU.  Offsets N(0, 0.6^2), everything else
    N(0, 1); per row a live-neighbour count uniform in 0..k, the slots past it exactly zero (the relfeat padding)."""
    g = torch.Generator().manual_seed(seed)
    ped = torch.randn(*lead, k, stride, generator=g)
    ped[..., :2] *= 0.6
    live = torch.randint(0, k + 1, lead, generator=g)
    ped = torch.where((torch.arange(k) < live[..., None])[..., None], ped, torch.zeros(()))
    vi, P, w = (torch.randn(*lead, 2, generator=g) for _ in range(3))
    return P, ped, vi, w


def decisions(P, ped, vi, thr=THR, dt=DT):
    """The correction's discrete choices and their margins in float64: (well-conditioned rows, {class: rows})."""
    P, ped, vi = (x.detach().double() for x in (P, ped, vi))
    k = ped.shape[-2]
    R = thr + 1.34 * 2 * dt
    inf = torch.tensor(float('inf'), dtype=torch.float64, device=P.device)
    p = torch.nan_to_num(ped[..., :2], nan=0.0)
    norm = torch.norm(p, p=2, dim=-1) + 1e-6
    nji = p / norm.unsqueeze(-1)
    w = ped[..., 2:4]
    vik = vi.unsqueeze(-2)
    inter = (vik * p).sum(-1) * ((w + vik) * (-p)).sum(-1)
    coll = (R >= norm) & (norm > 1e-4)
    enc, cha = coll & (inter > 0), coll & ~(inter > 0)
    ok = ((norm - R).abs() >= MARGIN).all(-1)
    ok &= (torch.where(coll, inter.abs(), inf) >= MARGIN).all(-1)
    ok &= ~(coll & (norm < NEAR)).any(-1)

    def nearest(flag):
        d = torch.where(flag, norm, inf).sort(dim=-1).values
        gap_ok = torch.ones_like(flag[..., 0]) if k < 2 else ~torch.isfinite(d[..., 1]) | (d[..., 1] - d[..., 0] >= MARGIN)
        idx = torch.where(flag, norm, inf).min(dim=-1).indices
        at = idx[..., None, None].expand(*idx.shape, 1, 2)
        return gap_ok, idx, torch.gather(nji, -2, at).squeeze(-2), torch.gather(w, -2, at).squeeze(-2)
    has_e, has_c = enc.any(-1), cha.any(-1)
    gap_e, idx_e, n1, _ = nearest(enc)
    gap_c, _, n2, w2 = nearest(cha)
    ok &= gap_e & gap_c
    s2 = (P * n1).sum(-1)
    ok &= ~has_e | (s2.abs() >= MARGIN)
    step2 = P - s2.clamp_min(0).unsqueeze(-1) * n1 - (vi * n1).sum(-1, keepdim=True) * n1 / dt
    P1 = torch.where(has_e.unsqueeze(-1), P + step2, P)
    q = (w2 * n2).sum(-1)
    ok &= ~has_c | (q.abs() >= MARGIN)
    act3 = has_c & (q < 0)
    s3 = (P1 * n2).sum(-1)
    ok &= ~act3 | (s3.abs() >= MARGIN)
    classes = {'neither': ~has_e & ~has_c, 'head-on only': has_e & ~has_c, 'chasing only': ~has_e & has_c,
               'both': has_e & has_c, 'step-2 s>0': has_e & (s2 > 0), 'step-2 s<=0': has_e & (s2 <= 0),
               'q<0': act3, 'q>=0': has_c & (q >= 0), 'step-3 s>0': act3 & (s3 > 0), 'step-3 s<=0': act3 & (s3 <= 0),
               'head-on not slot 0': has_e & (idx_e != 0), '>1 head-on': enc.sum(-1) > 1, '>1 chasing': cha.sum(-1) > 1}
    return ok, {name: rows & ok for name, rows in classes.items()}


K1_IMPOSSIBLE = ('both', 'head-on not slot 0', '>1 head-on', '>1 chasing')


def evaluate(fn, P, ped, vi, w, dtype, device, need=(True, True, True)):
    """(out, d/dP, d/dped, d/dvi) of sum(fn(...) * w); None for an input that does not require grad."""
    xs = [x.to(device=device, dtype=dtype).clone().requires_grad_(r) for x, r in zip((P, ped, vi), need)]
    out = fn(*xs)
    grads = torch.autograd.grad((out * w.to(device=device, dtype=dtype)).sum(), [x for x, r in zip(xs, need) if r])
    it = iter(grads)
    return [out.detach()] + [next(it) if r else None for r in need]


def kernel(P, ped, vi):
    from piml_amd import ops
    return ops.collision_post_correction(P, ped, vi, THR, DT)


def rel_err(got, ref, rows):
    got, ref = got.double().cpu()[rows.cpu()], ref.double().cpu()[rows.cpu()]
    return float((got - ref).abs().max() / ref.abs().max())


NAMES = ('output', 'd/d predictions', 'd/d ped_features', 'd/d velocity')
#         lead, k, stride, seed (the seeds chosen on the CPU for the conditions below: they use the float64 side alone)
CORRECTION_CASES = [((1000,), 6, 6, 0), ((257,), 1, 6, 0), ((513,), 10, 6, 0), ((3, 100), 3, 6, 1), ((2, 2, 65), 6, 9, 0),
                    ((1,), 6, 6, 87)]


@gpu
@pytest.mark.parametrize('lead,k,stride,seed', CORRECTION_CASES)
def test_correction_matches_float64(lead, k, stride, seed):
    """Forward and the analytic backward on the well-conditioned rows against float64 `torch_correction` + autograd:
    max |got - ref| / max |ref| per tensor.  The bar is 1e-5, or four times the error of `torch_correction` evaluated in
    float32 on the GPU where the kernel misses 1e-5 and that restatement itself exceeds 2.5e-6 (= max(1e-5, 4 x restatement)).

    Measured on the CPU (the float64 side alone decides them) -- rows left out, then the smallest class:
      (1000,) k=6: 0.8 %, 79 (>1 head-on);  (257,) k=1: 0.0 %, 6 (step-2 s<=0);  (513,) k=10: 1.9 %, 24 (head-on only);
      (3, 100) k=3: 0.7 %, 7 (>1 head-on);  (2, 2, 65) k=6 stride 9: 1.2 %, 19 (>1 head-on);  (1,): its row has both kinds.
    The float32 restatement against float64, evaluated on the CPU: at most 1.7e-7 (output), 1.0e-7 (d/d predictions),
    3.2e-7 (d/d ped_features), 2.2e-7 (d/d velocity) over the six cases, so the bar in force is expected to be 1e-5.
    NOT MEASURED YET: the kernel's own figures and the restatement's on the GPU (the test prints both per tensor)."""
    P, ped, vi, w = neighbourhoods(lead, k, stride, seed)
    ok, classes = decisions(P, ped, vi)
    counts = {name: int(rows.sum()) for name, rows in classes.items()}
    excluded = 1.0 - float(ok.double().mean())
    print(f'correction {lead} k={k} stride={stride}: excluded {100 * excluded:.1f} %, classes {counts}')
    if lead == (1,):
        assert bool(ok.all())
    else:
        assert excluded <= 0.05
        for name, n in counts.items():
            if not (k == 1 and name in K1_IMPOSSIBLE):
                assert n >= 5, (name, n)
    ref = evaluate(torch_correction, P, ped, vi, w, torch.float64, 'cpu')
    f32 = evaluate(torch_correction, P, ped, vi, w, torch.float32, DEV)
    got = evaluate(kernel, P, ped, vi, w, torch.float32, DEV)
    for name, a, b, c in zip(NAMES, got, f32, ref):
        e_kernel, e_f32 = rel_err(a, c, ok), rel_err(b, c, ok)
        bar = max(1e-5, 4 * e_f32)
        print(f'  {name}: kernel {e_kernel:.2e}, float32 restatement {e_f32:.2e} (bar {bar:.1e})')
        assert e_kernel <= bar, (name, e_kernel, e_f32)
    # features past the fourth are not read: other values there change nothing, and they receive exactly zero gradient
    other = ped.clone()
    other[..., 4:] = torch.where(ped[..., 4:] != 0, torch.randn(ped[..., 4:].shape, generator=torch.Generator().manual_seed(1)),
                                 torch.zeros(()))
    again = evaluate(kernel, P, other, vi, w, torch.float32, DEV)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    assert not got[2][..., 4:].any()


def test_single_row_case_is_well_conditioned():
    """The one-row parametrisation's seed, chosen on the CPU: its row is well-conditioned and has both kinds of neighbour."""
    lead, k, stride, seed = CORRECTION_CASES[-1]
    ok, classes = decisions(*neighbourhoods(lead, k, stride, seed)[:3])
    assert lead == (1,) and bool(ok.all()) and bool(classes['both'].all())


@gpu
@pytest.mark.parametrize('lead', [(300,), (2, 70), (1,)])
def test_correction_without_neighbours_is_identity(lead):
    """k == 0 (ped_features (..., N, 0, 6), handed over as a null pointer, which both entry points accept for k == 0): the
    output is the predictions, the upstream gradient passes through, the velocity receives zero."""
    g = torch.Generator().manual_seed(0)
    P, vi, w = (torch.randn(*lead, 2, generator=g) for _ in range(3))
    out, gP, gF, gV = evaluate(kernel, P, torch.zeros(*lead, 0, 6), vi, w, torch.float32, DEV)
    assert torch.equal(out.cpu(), P) and torch.equal(gP.cpu(), w)
    assert gF.shape == (*lead, 0, 6) and gV.shape == vi.shape and not gV.any()
    with torch.no_grad():
        assert torch.equal(kernel(P.to(DEV), torch.zeros(*lead, 0, 6, device=DEV), vi.to(DEV)).cpu(), P)


@gpu
def test_correction_gradients_one_at_a_time_and_deterministic():
    """Each gradient asked for alone is bit-equal to the one of the all-three call; two runs are bit-equal."""
    args = neighbourhoods((513,), 10, 6, 0)
    full = evaluate(kernel, *args, torch.float32, DEV)
    for a, b in zip(full, evaluate(kernel, *args, torch.float32, DEV)):
        assert torch.equal(a, b)
    for i in range(3):
        need = tuple(j == i for j in range(3))
        alone = evaluate(kernel, *args, torch.float32, DEV, need=need)
        assert torch.equal(alone[0], full[0]) and torch.equal(alone[1 + i], full[1 + i])
        assert all(alone[1 + j] is None for j in range(3) if j != i)


# Hand-built agents.  The focal agent moves with v_i = (1, 0); a neighbour at p = (0.5, +-0.25) (|p| = 0.559 < R = 0.7144) is
#   head-on  with v_ji = (-2, 0):   (v_i . p)(v_j . -p) = 0.5 * 0.5  > 0
#   chasing  with v_ji = (-0.5, 0): (v_i . p)(v_j . -p) = 0.5 * -0.25 < 0, and q = v_ji . n < 0 (the step acts)
VI = (1.0, 0.0)
HEAD_ON = (0.5, 0.25, -2.0, 0.0, 0.3, -0.7)
CHASING = (0.5, 0.25, -0.5, 0.0, -0.2, 0.9)
NAN = float('nan')
NAN_ROW = (NAN,) * 6


def mirrored(row):
    return (row[0], -row[1]) + tuple(row[2:])


def agents(*slots_per_agent):
    """(P, ped, vi, w) for hand-built agents: one tuple of neighbour rows per agent."""
    n = len(slots_per_agent)
    g = torch.Generator().manual_seed(5)
    P, w = torch.randn(n, 2, generator=g), torch.randn(n, 2, generator=g)
    P[:, 0] = P[:, 0].abs() + 0.5          # P . n > 0 for n ~ (0.89, +-0.45) whenever |P_y| stays small: both projections act
    P[:, 1] *= 0.25
    return P, torch.tensor(slots_per_agent, dtype=torch.float32), torch.tensor([VI] * n), w


def assert_close64(got, ref, what):
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a.isnan().cpu(), b.isnan()), (what, name, 'NaN positions')
        a, b = torch.nan_to_num(a.double().cpu()), torch.nan_to_num(b)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max().clamp_min(1.0)), (what, name)


@gpu
def test_correction_whole_nan_neighbour_row():
    """A neighbour row of six NaN next to a finite one, in both slot orders and for both kinds: never selected, the output is
    finite and bit-equal to the one with that row zeroed, its gradient entries are zero.  (The reference gathers slot 0 for a
    kind nobody is flagged for and multiplies by the kind's 0 mask afterwards, so a NaN row in slot 0 turns its whole agent NaN
    there; the kernel does not read an unflagged slot's velocity.)"""
    rows = [(HEAD_ON, NAN_ROW), (NAN_ROW, HEAD_ON), (CHASING, NAN_ROW), (NAN_ROW, CHASING)]
    P, ped, vi, w = agents(*rows)
    zeroed = torch.nan_to_num(ped, nan=0.0)
    got = evaluate(kernel, P, ped, vi, w, torch.float32, DEV)
    want = evaluate(kernel, P, zeroed, vi, w, torch.float32, DEV)
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert not got[2][ped.isnan().to(DEV)].any()
    assert not torch.equal(got[0].cpu(), P)                   # the finite neighbour was acted on
    assert_close64(got, evaluate(torch_correction, P, zeroed, vi, w, torch.float64, 'cpu'), 'NaN row zeroed')


@gpu
def test_correction_partially_nan_neighbour_rows():
    """Rows that are NaN in part, against float64 `torch_correction` + autograd (NaN positions equal, values through
    nan_to_num): a chasing neighbour with NaN relative velocity (q = NaN), and neighbours whose p_x is NaN and whose p_y alone
    places them inside the radius -- as the head-on and as the chasing row: p_x receives no gradient, p_y does."""
    vy = (0.0, 1.0)                                # with p = (NaN -> 0, 0.5): v_i . p = 0.5
    rows = [((0.5, 0.25, NAN, NAN, 0.0, 0.0), HEAD_ON[:1] + (-0.3,) + HEAD_ON[2:]),
            ((0.5, 0.25, -0.5, NAN, 0.0, 0.0), (0.0,) * 6),
            ((NAN, 0.5, 0.0, -2.0, 0.0, 0.0), (0.0,) * 6),          # head-on: v_j = (0, -1), (v_j . -p) = 0.5
            ((NAN, 0.5, 0.0, -0.5, 0.0, 0.0), (0.0,) * 6),          # chasing: v_j = (0, 0.5), q = -0.5
            ((0.0,) * 6, (NAN, 0.5, 0.0, -2.0, 0.0, 0.0)),
            ((NAN, 0.5, 0.0, -0.5, 0.0, 0.0), (NAN, -0.4, 0.0, -2.0, 0.0, 0.0))]     # chasing, and head-on from behind
    P, ped, vi, w = agents(*rows)
    vi[2:] = torch.tensor(vy)
    P[2:] = P[2:].flip(-1)                          # P . n > 0 for n = (0, 1)
    got = evaluate(kernel, P, ped, vi, w, torch.float32, DEV)
    ref = evaluate(torch_correction, P, ped, vi, w, torch.float64, 'cpu')
    assert bool(ref[0][:2].isnan().all()) and bool(torch.isfinite(ref[0][2:]).all())
    assert bool((ref[2][2:, :, 1].abs().sum(-1) > 0).all())             # p_y of a half-NaN row does receive gradient
    assert_close64(got, ref, 'partial NaN')
    # d n_y / d p_y at p = (0, p_y) is 1e-6 / (|p_y| + 1e-6)^2: the difference of two terms near 2, which float32 holds to a few
    # ulp of 2 (2.4e-7) in 4e-6 -- tens of per cent, and far below the tensor's scale above.  So: present, of the right sign and
    # within a factor of two; and exactly nothing for the NaN component.
    half_nan = ped[..., 0].isnan() & ~ped[..., 1].isnan()
    a, b = got[2].cpu()[half_nan], ref[2][half_nan]
    assert not a[:, 0].any() and not b[:, 0].any()
    assert bool(((a[:, 1] / b[:, 1] > 0.5) & (a[:, 1] / b[:, 1] < 2.0)).all()), (a[:, 1], b[:, 1])


@gpu
def test_correction_equidistant_neighbours_lower_slot_wins():
    """Two neighbours of one kind at exactly the same distance (mirrored offsets: equal float32 norms): torch.min's first
    minimum -- the lower slot -- is the selected one, forward and backward."""
    rows = [(HEAD_ON, mirrored(HEAD_ON)), (mirrored(HEAD_ON), HEAD_ON), (CHASING, mirrored(CHASING)),
            (mirrored(CHASING), CHASING)]
    P, ped, vi, w = agents(*rows)
    got = evaluate(kernel, P, ped, vi, w, torch.float32, DEV)
    first_only = ped.clone()
    first_only[:, 1] = 0
    ref = evaluate(torch_correction, P, first_only, vi, w, torch.float64, 'cpu')
    assert_close64(got, ref, 'equidistant')
    assert not got[2][:, 1].any() and bool(got[2][:, 0, :2].abs().sum(-1).min() > 0)
    other = evaluate(torch_correction, P, ped.flip(1), vi, w, torch.float64, 'cpu')
    assert float((other[0] - ref[0]).abs().max(-1).values.min()) > 1.0       # the other choice is a different answer


def f32_radius():
    """The radius as the entry point computes it: float(double(thr) + 1.34 * 2 * double(float(dt)))."""
    return np.float32(float(np.float32(THR)) + 1.34 * 2 * float(np.float32(DT)))


def boundary_offsets():
    """(p_in, p_out): adjacent float32 with fl(p_in + 1e-6f) == radius and fl(p_out + 1e-6f) > radius."""
    R, eps = f32_radius(), np.float32(1e-6)
    p = np.float32(R - eps)
    while np.float32(p + eps) > R:
        p = np.nextafter(p, np.float32(0))
    while np.float32(np.nextafter(p, np.float32(1)) + eps) <= R:
        p = np.nextafter(p, np.float32(1))
    return p, np.nextafter(p, np.float32(1))


def test_boundary_offsets_sit_on_the_radius():
    p_in, p_out = boundary_offsets()
    eps = np.float32(1e-6)
    assert np.float32(p_in + eps) == f32_radius() and np.float32(p_out + eps) > f32_radius()
    assert f32_radius() == np.float32(THR + 1.34 * 2 * DT)      # what float32 `torch_correction` compares with


@gpu
def test_correction_radius_boundary():
    """|p| + 1e-6f == radius in float32 is inside (>=), one ulp further is outside: float32 `torch_correction` is the
    reference for the decision itself (sqrt(fl(x * x)) == |x| makes the norm of (x, 0) exact on both sides)."""
    p_in, p_out = boundary_offsets()
    rows = [((float(p), 0.0) + HEAD_ON[2:], (0.0,) * 6) for p in (p_in, p_out, -p_in, -p_out)]
    P, ped, vi, w = agents(*rows)
    vi[2:] = -vi[2:]
    ped[2:, 0, 2] = 2.0
    got = evaluate(kernel, P, ped, vi, w, torch.float32, DEV)
    ref = evaluate(torch_correction, P, ped, vi, w, torch.float32, DEV)
    for name, a, b in zip(NAMES, got, ref):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max().clamp_min(1.0)), name
    out = got[0].cpu()
    assert torch.equal(out[1::2], P[1::2]) and bool(((out[0::2] - P[0::2]).abs().max(-1).values > 1.0).all())


# ------------------------------------------------------------------------------------------------
# 2. heading fill
# ------------------------------------------------------------------------------------------------
def norm_f32(x, y):
    """sqrt(fma(y, y, x * x)) in float32 (the float64 detour is exact for the fma), as test_selection_arithmetic_is_bit_exact."""
    f32, f64 = np.float32, np.float64
    with np.errstate(under='ignore', invalid='ignore', over='ignore'):
        xx = (np.asarray(x, f32) * np.asarray(x, f32)).astype(f32)
        return np.sqrt((xx.astype(f64) + np.asarray(y, f64) * np.asarray(y, f64)).astype(f32))


def heading_restated(velocity):
    """Pedestrians.get_heading_direction (src/data/data.py:350-395) for float32 (*c, T, N, 2): per (slice, agent) a sweep back
    and a sweep forward in time that put the last kept vector (initially +0) where the norm is zero -- the temporary is carried
    from the first sweep into the second -- then v / (n == 0 ? n + 0.1 : n)."""
    v = np.array(velocity, dtype=np.float32)
    T, N = v.shape[-3], v.shape[-2]
    h = v.reshape(-1, T, N, 2).copy()
    zero = norm_f32(h[..., 0], h[..., 1]) == 0
    for c in range(h.shape[0]):
        for i in range(N):
            if not zero[c, :, i].any():
                continue
            tmp = np.zeros(2, np.float32)
            for sweep in (range(T - 1, -1, -1), range(T)):
                for t in sweep:
                    if norm_f32(h[c, t, i, 0], h[c, t, i, 1]) == 0:
                        h[c, t, i] = tmp
                    else:
                        tmp = h[c, t, i].copy()
    n = norm_f32(h[..., 0], h[..., 1])
    n = np.where(n == 0, n + np.float32(0.1), n).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        return (h / n[..., None]).astype(np.float32).reshape(v.shape)


@pytest.mark.parametrize('name', golden_names('relfeat_'))
def test_heading_restatement_is_the_reference(name):
    """The restatement gives the reference's own `heading` arrays bit for bit (the inputs of test_heading_matches_reference_golden)."""
    g = golden(name)
    assert np.array_equal(bits(heading_restated(np.nan_to_num(g['velocity'], nan=0.0))), bits(g['heading']))


def heading_scene(shape, seed):
    """Velocities (*c, T, N, 2) whose agents stand (exact zeros of random sign) never / always / at the start / at the end /
    in the middle / every other frame, with a few entries of zero or subnormal squared norm and a few NaN."""
    rng = np.random.default_rng(seed)
    T, N = shape[-2:]
    C = int(np.prod(shape[:-2], dtype=np.int64))
    v = rng.standard_normal((C, T, N, 2)).astype(np.float32)
    pattern = rng.integers(0, 6, size=(C, N))
    t = np.arange(T)[None, :, None]
    a, b = rng.integers(0, T + 1, size=(2, C, 1, N))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    stand = [np.zeros((C, T, N), bool), np.ones((C, T, N), bool), t < np.maximum(lo, 1), t >= np.minimum(hi, T - 1),
             (t >= lo) & (t < hi), (t + a) % 2 == 0]
    standing = np.select([pattern[:, None, :] == q for q in range(6)], stand)
    signed_zero = np.where(rng.random(v.shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    v = np.where(standing[..., None], signed_zero, v)
    tiny = [(1e-30, 0.0), (1e-23, 1e-23), (3e-23, 3e-23)]       # x^2 + y^2 underflows to zero / to zero / to a subnormal
    for e in np.flatnonzero(rng.random(C * T * N) < 0.03):
        v.reshape(-1, 2)[e] = tiny[int(rng.integers(0, 3))]
    for e in np.flatnonzero(rng.random(C * T * N) < 0.02):
        v.reshape(-1, 2)[e, rng.integers(0, 3, size=1)[0] % 2] = np.nan          # one component ...
        if rng.random() < 0.3:
            v.reshape(-1, 2)[e] = np.nan                                         # ... or both
    return v.reshape(*shape, 2)


HEADING_SHAPES = [(1, 1), (1, 300), (7, 257), (3, 5, 64), (2, 2, 4, 33)]


def test_heading_scenes_hold_every_pattern():
    """The generator's content (CPU): every standing pattern, both zero signs, zero and subnormal norms, NaN entries."""
    seen = set()
    for q, shape in enumerate(HEADING_SHAPES):
        v = heading_scene(shape, q)
        n = norm_f32(v[..., 0], v[..., 1])
        z = (n == 0)
        seen |= {'-0.0'} if (np.signbit(v) & (v == 0)).any() else set()
        seen |= {'underflow'} if (z & (v != 0).any(-1)).any() else set()
        seen |= {'small norm'} if ((n > 0) & (n < 1e-20)).any() else set()
        seen |= {'nan one'} if (np.isnan(v).sum(-1) == 1).any() else set()
        seen |= {'nan both'} if (np.isnan(v).sum(-1) == 2).any() else set()
        if v.shape[-3] > 2:
            seen |= {'always'} if z.all(-2).any() else set()
            seen |= {'start'} if (z[..., 0, :] & ~z[..., -1, :]).any() else set()
            seen |= {'end'} if (~z[..., 0, :] & z[..., -1, :]).any() else set()
            seen |= {'middle'} if (~z[..., 0, :] & ~z[..., -1, :] & z.any(-2)).any() else set()
    assert seen == {'-0.0', 'underflow', 'small norm', 'nan one', 'nan both', 'always', 'start', 'end', 'middle'}


@gpu
@pytest.mark.parametrize('q,shape', list(enumerate(HEADING_SHAPES)))
def test_heading_fill_is_bit_exact(q, shape):
    """ops.heading_direction against the restatement: the same NaN positions, and every other output bit for bit."""
    from piml_amd import ops
    v = heading_scene(shape, q)
    want = heading_restated(v)
    got = ops.heading_direction(torch.tensor(v, device=DEV)).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    always = np.broadcast_to((norm_f32(v[..., 0], v[..., 1]) == 0).all(-2, keepdims=True), v.shape[:-1])
    assert not bits(got)[always].any()                        # +0.0 in every frame
    print(f'heading {shape}: {int(always[..., 0, :].sum())} agents always standing, {int(np.isnan(want).sum())} NaN outputs')


# ------------------------------------------------------------------------------------------------
# 3. the polar models against float64
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fused(on):
    import piml_amd.models.model as MODEL
    names = [n for n in vars(MODEL) if n.startswith('FUSED_') and isinstance(getattr(MODEL, n), bool)]
    saved = {n: getattr(MODEL, n) for n in names}
    try:
        for n in names:
            setattr(MODEL, n, on and saved[n])
        yield
    finally:
        for n, x in saved.items():
            setattr(MODEL, n, x)


@contextlib.contextmanager
def float64_operators(seen):
    """The module's own fallback path takes float64 everywhere but in its two float32-only operators.  For the float64
    evaluation they are `torch_correction` (whose inputs are recorded for the decision margins) and, since no velocity of
    these inputs is zero, a heading fill that has nothing to fill."""
    from piml_amd import ops
    saved = ops.collision_post_correction, ops.heading_direction

    def correction(P, ped, vi, thr, dt):
        seen.append((P.detach(), ped.detach(), vi.detach()))
        return torch_correction(P, ped, vi, thr, dt)

    def heading(v):
        n = torch.norm(v, p=2, dim=-1, keepdim=True)
        assert bool((n > 0).all())
        return v / n
    ops.collision_post_correction, ops.heading_direction = correction, heading
    try:
        yield
    finally:
        ops.collision_post_correction, ops.heading_direction = saved


def model_inputs(lead, seed):
    _, ped, _, _ = neighbourhoods(lead, 6, 6, seed)
    _, obs, _, _ = neighbourhoods(lead, 10, 6, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    sf = torch.randn(*lead, 7, generator=g)
    v = sf[..., 2:4]
    sin = v[..., 1] / v.norm(dim=-1)
    v[..., 1] = torch.where(sin.abs() < 0.05, torch.copysign(0.1 * v.norm(dim=-1), sin), v[..., 1])
    assert bool(((v[..., 1] / v.norm(dim=-1)).abs() >= 0.05).all())
    sf[..., 6] = 1.3 + 0.2 * sf[..., 6]
    return ped, obs, sf, torch.randn(*lead, 2, generator=g)


def model_run(m, ins, w, dtype, rows=None):
    xs = [x.to(device=DEV, dtype=dtype).clone().requires_grad_(True) for x in ins]
    out = m(*xs)[0]
    keep = torch.ones(out.shape[:-1], dtype=torch.bool, device=DEV) if rows is None else rows()
    loss = (out * w.to(device=DEV, dtype=dtype) * keep.unsqueeze(-1)).sum()
    return keep, [out.detach()] + list(torch.autograd.grad(loss, xs))


@gpu
@pytest.mark.parametrize('lead', [(300,), (3, 100)])
@pytest.mark.parametrize('name', ['pinnsf_pb', 'pinnsf_pbc'])
def test_polar_models_match_float64(name, lead):
    """Golden weights, eval(), the kernels the default dispatch takes: the acceleration and d(sum w * acceleration)/d(ped,
    obs, self features) against the module's own fallback path in float64 (see float64_operators), max |got - ref| /
    max |ref| per tensor.  For `pinnsf_pbc` the rows outside the well-conditioned set of the correction (margins from the
    float64 evaluation) are left out of the loss and of the output comparison.  The bar is four times the error of the
    float32 library path (FUSED_* off) against the same float64 evaluation, and below the 2e-3 of the golden test.

    The float64 side is the module's fallback path, not a restatement of the tail.
    NOT MEASURED YET: the test prints the fused kernels' and the library path's error per tensor."""
    m, _ = load(name)
    ins = model_inputs(lead, 11)
    w = ins[-1]
    m64, seen = copy.deepcopy(m).double(), []

    def well_conditioned():
        return decisions(*seen[-1])[0] if seen else torch.ones(lead, dtype=torch.bool, device=DEV)
    with fused(False), float64_operators(seen):
        rows, ref = model_run(m64, ins[:3], w, torch.float64, well_conditioned)
    assert (name == 'pinnsf_pbc') == bool(seen)
    excluded = 1.0 - float(rows.double().mean())
    with fused(False):
        _, lib = model_run(m, ins[:3], w, torch.float32, lambda: rows)
    _, got = model_run(m, ins[:3], w, torch.float32, lambda: rows)
    print(f'{name} {lead}: {100 * excluded:.1f} % of the rows left out')
    assert excluded <= 0.05
    every = torch.ones_like(rows)
    for what, a, b, c in zip(('acceleration', 'd/d ped', 'd/d obs', 'd/d self'), got, lib, ref):
        sel = rows if what == 'acceleration' else every
        e_kernel, e_lib = rel_err(a, c, sel), rel_err(b, c, sel)
        bar = 4 * e_lib
        print(f'  {what}: fused kernels {e_kernel:.2e}, float32 library path {e_lib:.2e} (bar {bar:.1e})')
        assert bar < 2e-3 and e_kernel <= bar, (what, e_kernel, e_lib)
