"""GPU: the neighbour search on tie-rich scenes (relfeat_tie_scenes.py; their preconditions: test_relfeat_tie_scenes.py) in every
launch form -- 4 / 8 / 16 waves, split and unsplit, resident, several agent or obstacle tiles, the LOCAL + REMOTE pair of a sharded
block, k at PIML_MAX_TOPK, more candidates than a wave's ring holds.  Every forward assertion is BITWISE against the CPU oracle
(oracle/piml_oracle.c: topk_in_sight): the selection is discrete.  Each case asserts, through piml_relfeat_plan (the rule the
launcher itself calls), the form it claims to cover and prints it.  The backward tests feed integer gradients, so that every sum
is exact whatever the order of the atomics: no tolerance."""
import numpy as np
import pytest
import torch

import relfeat_tie_scenes as TS
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')
STATE = ('position', 'velocity', 'acceleration', 'destination')


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def assert_form(name, want, **kw):
    got = TS.plan_of(name, **kw)
    print(f'\n[ties] {name} {TS.dims(name)} {kw or ""}: waves, resident, split, agent tiles, obstacle tiles = {got[1:]}')
    assert got[0] == 0 and got[1:1 + len(want)] == tuple(want), (name, got, want)


def assert_equals_oracle(out, ref, rows=None, what=''):
    """(ped_feat, obs_feat, dest_feat, ped_idx, obs_idx): features through bits(), indices as integers"""
    for n, (got, want) in enumerate(zip(out, ref[:5])):
        got = got.detach().cpu().numpy()
        want = want.reshape((-1,) + want.shape[want.ndim - got.ndim + 1:]) if rows is not None else want.reshape(got.shape)
        if rows is not None:
            want = want[rows]
        if got.dtype == np.int32:
            assert np.array_equal(got, want), (what, n, int((got != want).any(-1).sum()))
        else:
            assert np.array_equal(bits(got), bits(want)), (what, n)


def forward(name, **over):
    from piml_amd import ops
    sc = TS.scene(name)
    return ops.relative_features(*[dev(sc[k]) for k in STATE], dev(sc['obstacles']), return_index=True, **TS.geom(name, **over))


FORWARD = [
    # case, geometry overrides, (waves, resident, split[, agent tiles, obstacle tiles]) or None = the case's entry in TS.FORMS
    ('hall', {}, None),
    ('hall', dict(dist_threshold_ped=1.0, dist_threshold_obs=1.0), None),          # sources at exactly the threshold
    ('hall', dict(dist_threshold_ped=1.5, dist_threshold_obs=1.5), None),
    ('hall', dict(dist_threshold_ped=INF), None),
    ('hall', dict(sight_angle_ped=0, sight_angle_obs=180), None),                  # cosine threshold exactly 1.0 | nearly everything in view
    ('hall', TS.KMAX, None),                                                       # lanes 0 .. 31 of the list all live
    ('hall', dict(topk_ped=0), (8, 0, 0)),                                         # no pedestrian pass: unsplit
    ('hall_x2', {}, None),
    ('edge_4096', {}, None),
    ('edge_4097', {}, None),
    ('obstacle_tiles', {}, None),
    ('obstacle_tiles', dict(topk_obs=32, dist_threshold_obs=1.5), None),
    ('slices', {}, None),
    ('slices', TS.KMAX, None),
    ('slices', dict(topk_ped=0), (16, 1, 0)),
    ('slices', dict(dist_threshold_ped=1.0, sight_angle_ped=0, dist_threshold_obs=INF), None),
    ('many_slices', {}, None),
    ('small_600', {}, None),
    ('small_600', dict(sight_angle_ped=0, sight_angle_obs=0), None),
    ('small_1500', {}, None),
    ('small_1500', dict(dist_threshold_ped=1.5, sight_angle_ped=180), None),
    ('lattice_9000', {}, None),
    ('pile', {}, None),                                                            # > 1024 candidates per pass: the ring wraps
    ('pile', dict(topk_ped=32, topk_obs=32), None),
]


@pytest.mark.parametrize('name, over, form', FORWARD, ids=[f'{n}-{"-".join(f"{k}={v}" for k, v in o.items()) or "default"}' for n, o, _ in FORWARD])
def test_forward_equals_oracle_bitwise(oracle, name, over, form):
    assert_form(name, form or TS.FORMS[name], **over)
    out = forward(name, **over)
    ref = TS.reference(oracle, name, **over)
    assert_equals_oracle(out, ref, what=(name, over))
    if over == TS.KMAX:                                   # k at its bound: rows that fill all 32 slots, in both passes
        full = [int((t[..., 31] >= 0).sum()) for t in out[3:5]]
        print(f'[ties] {name}: rows with 32 live slots: pedestrians {full[0]}, obstacles {full[1]}')
        assert min(full) >= 100


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('over', [{}, TS.KMAX], ids=['default', 'kmax'])
def test_resident_kernels_of_four_and_eight_waves(oracle, monkeypatch, waves, over):
    """the slices again under PIML_RELFEAT_WAVES (read on every call): relfeat_fwd_kernel<4, true> and <8, true>"""
    monkeypatch.setenv('PIML_RELFEAT_WAVES', str(waves))
    assert_form('slices', (waves, 1, 0), **over)
    assert_equals_oracle(forward('slices', **over), TS.reference(oracle, 'slices', **over), what=('slices', waves))


@pytest.mark.parametrize('name', ['hall', 'hall_x2', 'pile'])
def test_three_wave_counts_agree_bitwise(oracle, monkeypatch, name):
    outs = []
    for waves in (4, 8, 16):
        monkeypatch.setenv('PIML_RELFEAT_WAVES', str(waves))
        assert_form(name, (waves,) + TS.FORMS[name][1:])
        outs.append(forward(name))
    ref = TS.reference(oracle, name)
    for out in outs:
        assert_equals_oracle(out, ref, what=name)
        for a, b in zip(out, outs[0]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_refused_wave_count_is_an_error_in_launcher_and_plan(monkeypatch):
    from piml_amd import _lib
    monkeypatch.setenv('PIML_RELFEAT_WAVES', '5')
    assert TS.plan_of('small_600')[0] == 1
    with pytest.raises(_lib.PimlHipError):
        forward('small_600')


@pytest.mark.parametrize('name', sorted(TS.BLOCKS))
def test_local_and_remote_parts_equal_one_launch_and_oracle(oracle, name):
    """relative_features_local_part + relative_features_packed_self(local=): the REMOTE launch restores the LOCAL list and then meets
    sources with LOWER indices that tie with its entries and must displace them."""
    from piml_amd import ops
    (f0, fc), local_form, remote_form = TS.BLOCKS[name]
    assert_form(name, local_form, part=1, focal_count=fc)
    assert_form(name, remote_form, part=2, focal_count=fc)
    sc, g = TS.scene(name), TS.geom(name)
    state = dev(np.concatenate([sc[k] for k in STATE[:3]], -1))
    d_rows, v0, obs = dev(sc['destination'][f0:f0 + fc]), dev(sc['desired_speed'][f0:f0 + fc]), dev(sc['obstacles'])
    one = ops.relative_features_packed_self(state, d_rows, obs, v0, f0, fc, return_index=True, **g)
    L = ops.relative_features_local_part(state, d_rows, obs, v0, f0, fc, want_grad=False, **g)
    local_list = L.ped_idx.clone()
    two = ops.relative_features_packed_self(state, d_rows, obs, v0, f0, fc, return_index=True, local=L, **g)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ref = TS.reference(oracle, name)
    for out in (one, two):
        assert_equals_oracle((out[0], out[1], out[2][:, :2].contiguous(), out[3], out[4]), ref, rows=slice(f0, f0 + fc), what=name)
    # the LOCAL list is the oracle's over the block's own agents, and the REMOTE part has work to do
    own = {k: sc[k][f0:f0 + fc] for k in STATE}
    ref_own = oracle.relfeat_fwd(*[own[k][None] for k in STATE], sc['obstacles'], return_index=True, **g)
    want_local = np.where(ref_own[3][0] >= 0, ref_own[3][0] + f0, -1)
    assert np.array_equal(local_list.cpu().numpy(), want_local)
    changed = int((local_list != two[3]).any(-1).sum())
    replaced = int(((local_list >= 0) & ~(local_list.unsqueeze(-1) == two[3].unsqueeze(-2)).any(-1)).all(-1).sum())
    print(f'[ties] {name} block [{f0}, {f0 + fc}): the REMOTE part changes {changed} of {fc} lists, replaces {replaced} whole')
    assert changed >= 100
    if name == 'pile':
        assert replaced == fc and bool((two[3] < f0).all())


@pytest.mark.parametrize('deterministic', [False, True], ids=['atomics', 'deterministic'])
@pytest.mark.parametrize('name', ['hall', 'slices', 'pile'])
def test_backward_is_exact_on_integer_gradients(oracle, name, deterministic):
    """relfeat_bwd (float atomics) and the sorted, atomics-free variant: the backward is a scatter-add with coefficients +-1, the
    upstream gradients are integers in [-8, 8], so every partial sum is an integer far below 2^24 (the pile sends ~1500 rows' terms
    to each of 12 sources: at most 1500 * 8) and both kernels must EQUAL the oracle's float64 sums."""
    from piml_amd import ops
    sc, g = TS.scene(name), TS.geom(name)
    rng = np.random.default_rng(5)
    leaves = [dev(sc[k]).requires_grad_(True) for k in STATE]
    try:
        ops.DETERMINISTIC_BWD = deterministic
        out = ops.relative_features(*leaves, dev(sc['obstacles']), return_index=True, **g)
        w = [rng.integers(-8, 9, size=tuple(t.shape)).astype(np.float32) for t in out[:3]]
        sum((o * dev(x)).sum() for o, x in zip(out[:3], w)).backward()
    finally:
        ops.DETERMINISTIC_BWD = False
    ref = TS.reference(oracle, name)
    assert_equals_oracle(out, ref, what=name)
    want = oracle.relfeat_bwd(w[0], w[1], w[2], ref[3].reshape(w[0].shape[:-1]), ref[4].reshape(w[1].shape[:-1]),
                              sc['position'], sc['destination'])
    top = max(float(np.abs(x).max()) for x in want)
    print(f'[ties] {name} backward ({"deterministic" if deterministic else "atomics"}): largest exact sum {top:.0f}')
    assert top < 2 ** 24 and top >= 8
    for leaf, x in zip(leaves, want):
        got = leaf.grad.cpu().numpy()
        assert np.array_equal(got, x.reshape(got.shape)), name
    absent = np.isnan(sc['position'][..., 0])
    for leaf in leaves:
        assert not leaf.grad.cpu().numpy()[absent].any()
    if name == 'pile':                                       # the longest run of equal keys: ~1500 rows name each of 12 sources
        counts = np.bincount(ref[3][ref[3] >= 0].ravel(), minlength=12)
        assert counts[:12].min() >= 1400
