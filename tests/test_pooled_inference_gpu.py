"""GPU: the pooled inference forward -- ops.fused_pinnsf_pooled, PIML_POOL_H2 of piml_pinnsf_fwd: enc_fwd_pool_x3_kernel,
dec_fwd_ph2_kernel and the desired-force epilogue -- against a float64 CPU restatement of the UNFOLDED model, at the edges of
its 32-row tiles.

Reference (`ref64`): per neighbour row the three-layer encoder (ReLU, ReLU, linear) times the processor scale, the sum over the
k rows, the decoder MLP(128, [64, 64]) and the predictor Linear(64, 2), summed over the branches, then the desired force
(v0 d / t - v) / tau with t = |d| per row and t + 0.1 where t == 0 (src/models/model.py:1289-1294 for flat input; the direct
operator always takes the per-row norm).  Plain torch float64 on copies of the module weights: it calls neither
ops.pooled_h2_decoder_weights nor any kernel nor the packed images -- the fold (W' = s Wd1 W3, b' = bd1 + s k Wd1 b3, made on
the host and packed as the decoder's first layer) is part of what is under test.

Bar: max |device - float64| <= 1e-5 x the largest magnitude of the float64 tensor, over ALL finite entries (the forward is
continuous: no agent is left out); the finite masks of both sides must be equal first, and nothing is passed through
nan_to_num.  Every case prints its worst ratio.

The shapes are chosen by property, and the property is asserted from N and k (TILE = 32 rows, served above MIN_TILES = 32
tiles in all): agent i straddles two tiles iff (k i) % 32 + k > 32.  The library's own serve / refuse answer at the first
served counts ties these two constants to the kernels."""
import functools

import pytest
import torch

from test_bench_step_gpu import BAR, _bits_equal, _compare
from test_mlpglue_gpu import model_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = 32             # rows per encoder tile (enc_fwd_pool_x3_kernel)
MIN_TILES = 32        # served above this many tiles over all branches (enc_pool_h2_ok)
H = 128
K_PED, K_OBS = 6, 10


# ---------------------------------------------------------------------------------------------------------
# tile arithmetic
# ---------------------------------------------------------------------------------------------------------
def tiles(N, k):
    return (N * k + TILE - 1) // TILE


def straddles(i, k):
    return (k * i) % TILE + k > TILE


def straddlers(N, k):
    return [i for i in range(N) if straddles(i, k)]


def served(N, ks):
    return sum(tiles(N, k) for k in ks) > MIN_TILES


def last_tile_agents(N, k):
    """agents with at least one row in the branch's last tile"""
    first_row = (tiles(N, k) - 1) * TILE
    return [i for i in range(N) if k * i + k - 1 >= first_row]


def ragged(N, k):
    return (N * k) % TILE != 0


# ---------------------------------------------------------------------------------------------------------
# inputs and weights
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_features(n_scene):
    """(ped (n, 6, 6), obs (n, 10, 6), self (n, 7)) of frame 0 of synthetic_rollout_data: the magnitudes the callers see"""
    from piml_amd.scenes import synthetic_rollout_data
    d = synthetic_rollout_data(n_scene, 2000, 1, DEV)
    out = tuple(t[0].contiguous() for t in (d.ped_features, d.obs_features, d.self_features))
    assert out[0].shape == (n_scene, K_PED, 6) and out[1].shape == (n_scene, K_OBS, 6) and out[2].shape == (n_scene, 7)
    for t in out:
        assert bool(torch.isfinite(t).all()), 'the synthetic scene left non-finite features'
    return out


def inputs(N):
    """The first N agents of a dense scene (4096 agents in the hall, or 16384: most neighbour slots are live).  The scene starts
    every agent at its desired velocity, where the desired force vanishes: the velocities are turned and slowed here (same
    magnitudes), and every 37th agent stands on its destination (|d| == 0: the t + 0.1 branch)."""
    pf, of, sf = [t[:N].clone() for t in _scene_features(4096 if N <= 4096 else 16384)]
    i = torch.arange(N, device=DEV, dtype=torch.float32)
    vx, vy = sf[:, 2].clone(), sf[:, 3].clone()
    c, s = torch.cos(0.7 * i), torch.sin(0.7 * i)
    sf[:, 2], sf[:, 3] = 0.8 * (c * vx - s * vy), 0.8 * (s * vx + c * vy)
    sf[::37, :2] = 0.0
    return pf, of, sf


def make_model(seed=666, **kw):
    import piml_amd.models.model as MODEL
    torch.manual_seed(seed)
    return MODEL.PINNSF(model_args(**kw)).to(DEV).eval()


def branch_weights(m, name):
    """(encoder w1 b1 w2 b2 w3 b3, decoder w1 b1 w2 b2, predictor w b) of branch 'ped' / 'obs'"""
    enc, dec, pred = getattr(m, name + '_encoder'), getattr(m, name + '_decoder'), getattr(m, name + '_predictor')
    return ([t for lin in enc.mlp[0::2] for t in (lin.weight, lin.bias)],
            [t for lin in dec.mlp[0::2] for t in (lin.weight, lin.bias)], [pred.mlp[0].weight, pred.mlp[0].bias])


def eval_scale(m, name):
    scale, keep = getattr(m, name + '_processor').fused_spec(1, torch.device(DEV))
    assert keep is None and scale == 2.0
    return scale


# ---------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------
def ref64(ws, xs, sf, scales, tau, epilogue=True):
    """(acc (..., 2), [h2 (..., k, 128) per branch]) of the unfolded model in float64 on the CPU."""
    acc, h2s = 0.0, []
    for (e, d, p), x, s in zip(ws, xs, scales):
        e, d, p = [[t.detach().double().cpu() for t in grp] for grp in (e, d, p)]
        x = x.detach().double().cpu()
        h1 = torch.relu(x @ e[0].t() + e[1])
        h2 = torch.relu(h1 @ e[2].t() + e[3])
        msgs = float(s) * (h2 @ e[4].t() + e[5])
        pooled = msgs.sum(-2)
        dec = torch.relu(pooled @ d[0].t() + d[1]) @ d[2].t() + d[3]
        acc = acc + dec @ p[0].t() + p[1]
        h2s.append(h2)
    if epilogue:
        f = sf.detach().double().cpu()
        t = torch.norm(f[..., :2], p=2, dim=-1, keepdim=True)
        t = torch.where(t == 0, t + 0.1, t)
        acc = acc + (f[..., 6:7] * (f[..., :2] / t) - f[..., 2:4]) / float(tau)
    return acc, h2s


def report(name, got, want):
    ratio = _compare(name, got, want)
    print(f'\n{name}: {ratio:.3e} of the largest float64 magnitude (bar {BAR:.0e})')
    assert ratio <= BAR, f'{name}: differs from float64 by {ratio:.3e} of its largest magnitude (bar {BAR:.0e})'
    return ratio


# ---------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------
def folded(ws, xs, scales):
    """(encoder weights, folded decoder + predictor weights) per branch, as PINNSF._pooled_inference makes them"""
    from piml_amd import ops
    enc_w = [list(e) for e, _, _ in ws]
    dec_w = [ops.pooled_h2_decoder_weights(e, [*d, *p], s, x.shape[-2]) for (e, d, p), x, s in zip(ws, xs, scales)]
    return enc_w, dec_w


def pooled(ws, xs, sf, scales, tau, epilogue=True, packed=True):
    """ops.fused_pinnsf_pooled on the folded weights (None: refused)"""
    from piml_amd import ops
    enc_w, dec_w = folded(ws, xs, scales)
    packs = None
    if packed:
        packs = ops.PinnsfPacks()
        ops.pinnsf_prepack(packs, enc_w, dec_w, None, defer=False)
    with torch.no_grad():
        out = ops.fused_pinnsf_pooled([dict(x=x, encoder=ew, decoder=dw) for x, ew, dw in zip(xs, enc_w, dec_w)],
                                      sf, tau, fold_epilogue=epilogue, packs=packs)
    torch.cuda.synchronize()
    return out


def direct(ws, xs, sf, scales, tau, packed, fill):
    """piml_pinnsf_fwd with PIML_POOL_H2 on buffers of the test's own, every one pre-filled with `fill`; the structs built the
    way ops.fused_pinnsf_pooled builds them.  Returns (acc, part_a per branch, part_b per branch)."""
    from piml_amd import _lib, ops
    L = _lib.lib()
    nbr, agents = len(xs), xs[0].shape[0]
    opt = dict(device=DEV, dtype=torch.float32)
    enc_w, dec_w = folded(ws, xs, scales)
    enc_w = [[t.detach().contiguous() for t in wb] for wb in enc_w]
    x2s = [x.reshape(-1, x.shape[-1]).contiguous() for x in xs]
    ks = [x.shape[-2] for x in xs]
    flags = _lib.POOL_H2
    if packed:
        packs = ops.PinnsfPacks()
        ops.pinnsf_prepack(packs, enc_w, dec_w, None, defer=False)
        epack, dpack = packs.epack, packs.dpack
        flags |= _lib.PACKED_VALID
    else:
        epack = torch.empty(nbr, L.piml_encoder_pack_floats(), **opt)
        dpack = torch.empty(nbr, L.piml_decoder_pack_floats(), **opt)
    part_a = [torch.full((agents, H), fill, **opt) for _ in range(nbr)]
    part_b = [torch.full((agents, H), fill, **opt) for _ in range(nbr)]
    acc = torch.full((agents, 2), fill, **opt)
    earr = (_lib.EncoderBranch * nbr)(*[ops._enc_branch_struct(x2s[b], ks[b], 1.0, enc_w[b], part_a[b], None, part_b[b], packed=epack[b])
                                        for b in range(nbr)])
    assert L.piml_pinnsf_pool_h2_ok(earr, nbr) == 1
    darr = (_lib.DecoderBranch * nbr)(*[ops._dec_branch_struct(part_b[b], agents, ks[b], dec_w[b], dpack[b], part_a[b], None, None)
                                        for b in range(nbr)])
    sfc = sf.contiguous()
    with torch.cuda.device(torch.device(DEV)):
        _lib.check(L.piml_pinnsf_fwd(earr, darr, nbr, None, ops._ptr(sfc), float(tau), ops._ptr(acc), flags, ops._stream()),
                   'piml_pinnsf_fwd')
    torch.cuda.synchronize()
    return acc, part_a, part_b


@pytest.fixture(scope='module')
def net():
    """the seeded default-init network (128 / 128 / 64), its two branches' weights and eval-mode scales"""
    m = make_model()
    ws = [branch_weights(m, 'ped'), branch_weights(m, 'obs')]
    return m, ws, [eval_scale(m, 'ped'), eval_scale(m, 'obs')]


# ---------------------------------------------------------------------------------------------------------
# 1. direct call, poisoned buffers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', [float('nan'), 1e30], ids=['nan', '1e30'])
@pytest.mark.parametrize('packed', [False, True], ids=['POOL_H2', 'POOL_H2+PACKED_VALID'])
def test_direct_call_into_poisoned_buffers(net, packed, fill):
    """part_a / part_b / acc are the test's own tensors, pre-filled with NaN or 1e30.  Every acc entry is finite and within the
    bar (so the decoder read no second part of a non-straddler and the encoder skipped no part), every agent's first part and
    every STRADDLER's second part equals the float64 sum of h2 over its rows in that tile; a non-straddler's second part is
    unspecified and not read here."""
    m, ws, scales = net
    N = 203                       # both branches ragged, straddlers in both, the last pedestrian agent one of them
    assert ragged(N, K_PED) and ragged(N, K_OBS) and straddles(N - 1, K_PED) and served(N, (K_PED, K_OBS))
    pf, of, sf = inputs(N)
    acc, part_a, part_b = direct(ws, [pf, of], sf, scales, m.tau, packed, fill)
    want, h2s = ref64(ws, [pf, of], sf, scales, m.tau)
    assert bool(torch.isfinite(acc).all()), f'{int((~torch.isfinite(acc)).sum())} acc entries are not finite'
    tag = f'direct[{"packed" if packed else "in-call pack"}, fill {fill}]'
    report(f'{tag} acc', acc, want)
    for b, k in enumerate((K_PED, K_OBS)):
        S = straddlers(N, k)
        assert S and len(S) < N
        first = torch.tensor([min(k, TILE - (k * i) % TILE) for i in range(N)])         # rows of agent i in its first tile
        in_a = (torch.arange(k)[None, :] < first[:, None]).double()[..., None]           # (N, k, 1)
        want_a, want_b = (h2s[b] * in_a).sum(1), (h2s[b] * (1 - in_a)).sum(1)
        assert [i for i in range(N) if first[i] < k] == S
        report(f'{tag} branch {b} first parts (all {N} agents)', part_a[b], want_a)
        report(f'{tag} branch {b} second parts ({len(S)} straddlers)', part_b[b][S], want_b[S])


# ---------------------------------------------------------------------------------------------------------
# 2. shapes, two branches
# ---------------------------------------------------------------------------------------------------------
def _one_agent_last_tiles(N):
    return last_tile_agents(N, K_PED) == [N - 1] and last_tile_agents(N, K_OBS) == [N - 1] and not served(N - 1, (K_PED, K_OBS))


SHAPES = [
    (65, 'first served count, one agent in each last tile', _one_agent_last_tiles),
    (75, 'last pedestrian agent straddles into a partial tile', lambda N: straddles(N - 1, K_PED) and ragged(N, K_PED)),
    (77, 'last obstacle agent straddles into a partial tile', lambda N: straddles(N - 1, K_OBS) and ragged(N, K_OBS)),
    (512, 'no ragged tile', lambda N: not ragged(N, K_PED) and not ragged(N, K_OBS)),
    (3001, 'thousands, ragged', lambda N: N % 16 != 0 and ragged(N, K_PED) and ragged(N, K_OBS)),
    (16384, 'the cfg4 scene', lambda N: not ragged(N, K_PED)),
]


@pytest.mark.parametrize('N,what,prop', SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_two_branches_match_float64(net, N, what, prop):
    m, ws, scales = net
    assert prop(N), f'N = {N} no longer has the property "{what}"'
    assert served(N, (K_PED, K_OBS))
    assert tiles(65, K_PED) + tiles(65, K_OBS) == 34 and tiles(64, K_PED) + tiles(64, K_OBS) == 32
    assert N % 16 not in (11, 6) or straddles(N - 1, K_PED)
    assert N % 16 not in (13, 10, 7, 4) or straddles(N - 1, K_OBS)
    pf, of, sf = inputs(N)
    got = pooled(ws, [pf, of], sf, scales, m.tau)
    assert got is not None, f'N = {N} ({what}) was refused'
    report(f'two branches, N = {N} ({what})', got, ref64(ws, [pf, of], sf, scales, m.tau)[0])


# ---------------------------------------------------------------------------------------------------------
# 3. one branch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,k', [(171, 6), (1003, 6), (1003, 10), (103, 10)])
def test_one_branch_matches_float64(net, N, k):
    """nbr = 1 (the obstacle-free crosswalk): k = 6 from its first served count (171 agents = 33 tiles; 170 = 32 is refused) and a
    larger ragged count, and k = 10 alone (first served count 103: 1030 rows = 33 tiles)."""
    m, ws, scales = net
    assert served(N, (k,)) and ragged(N, k)
    assert tiles(171, 6) == 33 and tiles(170, 6) == 32 and tiles(103, 10) == 33 and tiles(102, 10) == 32
    pf, of, sf = inputs(N)
    b = 0 if k == K_PED else 1
    x = (pf, of)[b]
    got = pooled(ws[b:b + 1], [x], sf, scales[b:b + 1], m.tau)
    assert got is not None
    report(f'one branch, k = {k}, N = {N}', got, ref64(ws[b:b + 1], [x], sf, scales[b:b + 1], m.tau)[0])


# ---------------------------------------------------------------------------------------------------------
# 4. other input widths
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_dim', [1, 3, 8])
def test_other_input_width(net, in_dim):
    """pedestrian encoder of in_dim 1, 3, 8 beside the 6-wide obstacle encoder, on a ragged shape"""
    m, ws, scales = net
    N = 203
    assert ragged(N, K_PED) and ragged(N, K_OBS)
    m2 = make_model(seed=7, ped_feature_dim=in_dim)
    assert m2.ped_encoder.mlp[0].weight.shape == (H, in_dim)
    ws2 = [branch_weights(m2, 'ped'), ws[1]]
    pf, of, sf = inputs(N)
    pf = torch.cat((pf, pf[..., :2]), -1)[..., :in_dim].contiguous()
    got = pooled(ws2, [pf, of], sf, scales, m.tau)
    assert got is not None
    report(f'in_dim = {in_dim}, N = {N}', got, ref64(ws2, [pf, of], sf, scales, m.tau)[0])


# ---------------------------------------------------------------------------------------------------------
# 5. lead shapes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lead', [(3, 50), (32, 61)])
def test_lead_shapes_equal_the_flat_call(net, lead):
    """(C, N) / (members, capacity) input: bitwise the flat call, and within the bar of float64 (per-row norm in both)."""
    m, ws, scales = net
    N = lead[0] * lead[1]
    assert served(N, (K_PED, K_OBS))
    pf, of, sf = inputs(N)
    flat = pooled(ws, [pf, of], sf, scales, m.tau)
    got = pooled(ws, [pf.view(*lead, K_PED, 6), of.view(*lead, K_OBS, 6)], sf.view(*lead, 7), scales, m.tau)
    assert got.shape == (*lead, 2) and flat.shape == (N, 2)
    assert _bits_equal(got.reshape(N, 2), flat), f'lead {lead}: not the bits of the flat call'
    report(f'lead shape {lead}', got, ref64(ws, [pf, of], sf, scales, m.tau)[0].view(*lead, 2))


# ---------------------------------------------------------------------------------------------------------
# 6. fold_epilogue
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nbr', [1, 2])
def test_fold_epilogue_both_ways(net, nbr):
    """fold_epilogue=False hands piml_pinnsf_fwd a NULL self_features: the result is the sum of the branches' predictor
    outputs (bias included) and nothing else -- no desired force, self_features not read.  True adds (v0 d / t - v) / tau."""
    m, ws, scales = net
    N = 203
    pf, of, sf = inputs(N)
    xs = [pf, of][:nbr]
    bare = pooled(ws[:nbr], xs, sf, scales[:nbr], m.tau, epilogue=False)
    full = pooled(ws[:nbr], xs, sf, scales[:nbr], m.tau, epilogue=True)
    poisoned = pooled(ws[:nbr], xs, torch.full_like(sf, float('nan')), scales[:nbr], m.tau, epilogue=False)
    assert _bits_equal(bare, poisoned), 'fold_epilogue=False read self_features'
    report(f'fold_epilogue=False, {nbr} branch(es)', bare, ref64(ws[:nbr], xs, sf, scales[:nbr], m.tau, epilogue=False)[0])
    report(f'fold_epilogue=True, {nbr} branch(es)', full, ref64(ws[:nbr], xs, sf, scales[:nbr], m.tau, epilogue=True)[0])
    assert float((full - bare).abs().max()) > 1e-2          # the two differ by the desired force, far beyond the bar


# ---------------------------------------------------------------------------------------------------------
# 7. refusals and fallback
# ---------------------------------------------------------------------------------------------------------
def test_refused_configurations(net):
    """Below the tile bound, k = 7 and in_dim = 9 return None from ops.fused_pinnsf_pooled (no error, nothing launched); a row
    count that is not a multiple of k cannot be expressed through the operator (x is (..., N, k, in)) and is refused by the
    library's own test, piml_pinnsf_pool_h2_ok."""
    from piml_amd import _lib, ops
    m, ws, scales = net
    assert not served(64, (K_PED, K_OBS)) and served(65, (K_PED, K_OBS))
    assert not served(170, (K_PED,)) and served(171, (K_PED,))
    pf, of, sf = inputs(203)
    assert pooled(ws, [pf[:64], of[:64]], sf[:64], scales, m.tau) is None
    assert pooled(ws, [pf[:65], of[:65]], sf[:65], scales, m.tau) is not None
    assert pooled(ws[:1], [pf[:170]], sf[:170], scales[:1], m.tau) is None
    assert pooled(ws[:1], [pf[:171]], sf[:171], scales[:1], m.tau) is not None
    assert pooled(ws[1:], [of[:102]], sf[:102], scales[1:], m.tau) is None
    # k = 7: enough rows, another neighbour count
    pf7 = torch.cat((pf, pf[:, :1]), 1).contiguous()
    assert pf7.shape == (203, 7, 6) and tiles(203, 7) + tiles(203, K_OBS) > MIN_TILES
    assert pooled(ws, [pf7, of], sf, scales, m.tau, packed=False) is None
    # in_dim = 9
    m9 = make_model(seed=9, ped_feature_dim=9)
    pf9 = torch.cat((pf, pf[..., :3]), -1).contiguous()
    assert pooled([branch_weights(m9, 'ped'), ws[1]], [pf9, of], sf, scales, m.tau, packed=False) is None
    # rows not a multiple of k, asked of the library directly
    L = _lib.lib()
    arr = (_lib.EncoderBranch * 1)()
    arr[0].in_dim, arr[0].k = 6, K_PED
    for rows, ok in ((171 * K_PED, 1), (171 * K_PED + 1, 0), (172 * K_PED - 1, 0), (170 * K_PED, 0)):
        arr[0].rows = rows
        assert L.piml_pinnsf_pool_h2_ok(arr, 1) == ok, f'rows = {rows}, k = {K_PED}'


def _spy(monkeypatch, obj, name, log):
    orig = getattr(obj, name)

    def wrapper(*a, **kw):
        out = orig(*a, **kw)
        log.append((name, out))
        return out
    monkeypatch.setattr(obj, name, wrapper)


def _model_frame(m, pf, of, sf):
    return m(pf, of, sf)[0]


@pytest.mark.parametrize('N', [170, 171])
def test_model_falls_back_to_the_message_path(monkeypatch, N):
    """PINNSF.forward (predictions only, inside packed_weights()) of the one-branch model: 171 agents are served by the pooled
    path (model._ph2 set), 170 are refused by it (32 tiles) and served by ops.fused_pinnsf -- both within the bar of the
    same float64 reference.  (Two branches cannot be refused through the model: its fused network starts at 512 pedestrian
    rows, 86 agents, which is 44 tiles.)"""
    from piml_amd import ops
    m = make_model(obs_feature_dim=0)
    ws, scales = [branch_weights(m, 'ped')], [eval_scale(m, 'ped')]
    pf, _, sf = inputs(N)
    none = torch.empty(0, device=DEV)
    log = []
    _spy(monkeypatch, ops, 'fused_pinnsf_pooled', log)
    _spy(monkeypatch, ops, 'fused_pinnsf', log)
    m.predictions_only = True
    with torch.no_grad(), m.packed_weights():
        got = _model_frame(m, pf, none, sf)
        assert m._ph2 is not None              # the fold is made before the library is asked (kept for a later, larger frame)
    assert m._ph2 is None
    if served(N, (K_PED,)):
        assert [n for n, _ in log] == ['fused_pinnsf_pooled'] and log[0][1] is not None
    else:
        assert [n for n, _ in log] == ['fused_pinnsf_pooled', 'fused_pinnsf'] and log[0][1] is None
    report(f'model, one branch, N = {N} ({"pooled" if served(N, (K_PED,)) else "refused: message path"})', got,
           ref64(ws, [pf], sf, scales, m.tau)[0])


# ---------------------------------------------------------------------------------------------------------
# 8. NaN / Inf containment
# ---------------------------------------------------------------------------------------------------------
def test_nan_and_inf_stay_in_their_agents(net):
    """NaN in all k pedestrian rows of a few agents (a straddler whose neighbours in both tiles stay clean; a straddler AND the
    agent after it), NaN in other agents' self_features, Inf in one more agent's: exactly those agents have non-finite
    outputs -- the finite mask equals float64's entry by entry -- and every other agent meets the bar against the float64
    reference of the same poisoned input.
    (What this case found: the kernels' one-instruction ReLUs answer 0 to a NaN, so an agent with NaN feature rows came out with
    a FINITE acceleration; enc_fwd_pool_x3_kernel and dec_fwd_body now carry the NaN through their ReLUs.)"""
    m, ws, scales = net
    N = 203
    S = straddlers(N, K_PED)
    s1, s2 = S[3], S[9]
    assert straddles(s1, K_PED) and not straddles(s1 + 1, K_PED) and (K_PED * (s1 + 1)) // TILE == (K_PED * s1 + K_PED - 1) // TILE
    assert straddles(s2, K_PED) and (K_PED * (s2 + 1)) // TILE == (K_PED * s2 + K_PED - 1) // TILE
    nan_feat = [7, s1, s2, s2 + 1, N - 1]              # (7: no straddler; N - 1: the last agent, a straddler into the ragged tile)
    nan_self = {17: 0, 40: 6, 121: 3}                   # agent: column of self_features
    inf_self = {150: 2}
    poisoned = sorted(set(nan_feat) | set(nan_self) | set(inf_self))
    assert len(poisoned) == len(nan_feat) + len(nan_self) + len(inf_self) and s1 - 1 not in poisoned and s1 + 1 not in poisoned
    pf, of, sf = inputs(N)
    pf[nan_feat] = float('nan')
    for a, c in nan_self.items():
        sf[a, c] = float('nan')
    for a, c in inf_self.items():
        sf[a, c] = float('inf')
    got = pooled(ws, [pf, of], sf, scales, m.tau)
    want = ref64(ws, [pf, of], sf, scales, m.tau)[0]
    bad_got = (~torch.isfinite(got)).any(-1).nonzero().flatten().tolist()
    bad_want = (~torch.isfinite(want)).any(-1).nonzero().flatten().tolist()
    assert bad_want == poisoned
    assert bad_got == poisoned, f'non-finite outputs at agents {bad_got}, poisoned were {poisoned}'
    assert torch.equal(torch.isfinite(got).cpu(), torch.isfinite(want)), 'finite masks differ from float64 inside the poisoned agents'
    report(f'NaN / Inf containment, N = {N} ({N - len(poisoned)} clean agents)', got, want)


# ---------------------------------------------------------------------------------------------------------
# 9. absent agents
# ---------------------------------------------------------------------------------------------------------
def test_all_zero_feature_rows(net):
    """Agents whose feature rows are all zero in both branches (what relfeat writes for dead neighbour slots), with finite
    self_features: the rows' h2 is the encoders' bias response, the same for all k rows, so the folded bias b' = bd1 + s k Wd1 b3
    carries its largest share here.  Compared on those agents alone as well."""
    m, ws, scales = net
    N = 203
    pf, of, sf = inputs(N)
    zero = sorted(set(straddlers(N, K_PED)[:4] + straddlers(N, K_OBS)[:4] + [0, 1, 2, 100, N - 1]))
    pf[zero] = 0.0
    of[zero] = 0.0
    got = pooled(ws, [pf, of], sf, scales, m.tau)
    want = ref64(ws, [pf, of], sf, scales, m.tau)[0]
    report(f'all-zero rows, all {N} agents', got, want)
    bare = pooled(ws, [pf, of], sf, scales, m.tau, epilogue=False)
    want_bare = ref64(ws, [pf, of], sf, scales, m.tau, epilogue=False)[0]
    report(f'all-zero rows, the {len(zero)} zeroed agents alone, no desired force', bare[zero], want_bare[zero])
    assert float((want_bare[zero] - want_bare[zero][0]).abs().max()) < 1e-12        # one value: the network's response to no neighbour


# ---------------------------------------------------------------------------------------------------------
# 10. repeatability
# ---------------------------------------------------------------------------------------------------------
def test_repeatable_eager_and_replayed(net):
    from piml_amd import ops
    m, ws, scales = net
    N = 3001
    pf, of, sf = inputs(N)
    enc_w, dec_w = folded(ws, [pf, of], scales)
    packs = ops.PinnsfPacks()
    ops.pinnsf_prepack(packs, enc_w, dec_w, None, defer=False)
    branches = [dict(x=x, encoder=ew, decoder=dw) for x, ew, dw in zip((pf, of), enc_w, dec_w)]
    with torch.no_grad():
        a = ops.fused_pinnsf_pooled(branches, sf, m.tau, packs=packs)
        b = ops.fused_pinnsf_pooled(branches, sf, m.tau, packs=packs)
        c = ops.fused_pinnsf_pooled(branches, sf, m.tau, packs=None)
        torch.cuda.synchronize()
        assert _bits_equal(a, b), 'two eager calls differ'
        assert _bits_equal(a, c), 'the call that packs for itself differs from the call on prepacked images'
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.fused_pinnsf_pooled(branches, sf, m.tau, packs=packs)
        for r in range(3):
            out.fill_(float('nan'))
            g.replay()
            torch.cuda.synchronize()
            assert _bits_equal(out, a), f'replay {r} differs from the eager call'
    report(f'repeatability, N = {N}', a, ref64(ws, [pf, of], sf, scales, m.tau)[0])


# ---------------------------------------------------------------------------------------------------------
# 11. the cached fold, through the model
# ---------------------------------------------------------------------------------------------------------
def _model_ws(m):
    return [branch_weights(m, 'ped'), branch_weights(m, 'obs')], [eval_scale(m, 'ped'), eval_scale(m, 'obs')]


def test_fold_follows_the_weights():
    """Two frames of one packed_weights() block give equal bits; after an in-place update of every parameter a new block gives
    the float64 result of the NEW weights, which is far from the old one."""
    m = make_model(seed=11)
    N = 203
    pf, of, sf = inputs(N)
    m.predictions_only = True
    with torch.no_grad():
        with m.packed_weights():
            a = _model_frame(m, pf, of, sf)
            assert m._ph2 is not None and m._ph2.key == ((K_PED, K_OBS), (2.0, 2.0))
            b = _model_frame(m, pf, of, sf)
        assert m._ph2 is None
        torch.cuda.synchronize()
        assert _bits_equal(a, b)
        ws, scales = _model_ws(m)
        old = ref64(ws, [pf, of], sf, scales, m.tau)[0]
        report('model, first block', a, old)
        g = torch.Generator(device=DEV).manual_seed(5)
        for p in m.parameters():
            p.add_(0.01 * torch.randn(p.shape, device=DEV, generator=g))
        with m.packed_weights():
            c = _model_frame(m, pf, of, sf)
            assert m._ph2 is not None
        torch.cuda.synchronize()
    new = ref64(ws, [pf, of], sf, scales, m.tau)[0]           # (ws are the parameters themselves: updated in place)
    moved = float((new - old).abs().max() / new.abs().max())
    print(f'\nthe update moved the float64 result by {moved:.3e} of its largest magnitude')
    assert moved > 1000 * BAR
    report('model, new block after the weight update', c, new)


def test_other_k_inside_one_block_rebuilds_the_fold():
    """A frame with 10 pedestrian neighbours after a frame with 6, inside one block: the fold's key changes, the fold is made
    again with k = 10 in b' and the frame is served within the bar (the stale fold would be off by 4 s Wd1 b3)."""
    m = make_model(seed=12)
    N = 203
    pf, of, sf = inputs(N)
    pf10 = torch.cat((pf, 0.5 * pf[:, :4]), 1).contiguous()
    assert pf10.shape == (N, 10, 6)
    ws, scales = _model_ws(m)
    m.predictions_only = True
    with torch.no_grad(), m.packed_weights():
        a = _model_frame(m, pf, of, sf)
        first = m._ph2
        assert first.key[0] == (K_PED, K_OBS)
        b = _model_frame(m, pf10, of, sf)
        assert m._ph2 is not first and m._ph2.key[0] == (10, K_OBS)
        c = _model_frame(m, pf, of, sf)
        assert m._ph2.key[0] == (K_PED, K_OBS)
        torch.cuda.synchronize()
    report('k = 6 frame', a, ref64(ws, [pf, of], sf, scales, m.tau)[0])
    want10 = ref64(ws, [pf10, of], sf, scales, m.tau)[0]
    report('k = 10 frame inside the same block', b, want10)
    assert _bits_equal(a, c), 'back at k = 6: not the bits of the first frame'


def test_capture_without_a_fold_takes_the_message_path(monkeypatch):
    """Under stream capture with no fold cached _pooled_inference returns None (the fold's host work cannot be captured) and
    the message path serves the captured frame, within the bar."""
    import piml_amd.models.model as MODEL
    m = make_model(seed=13)
    N = 203
    pf, of, sf = inputs(N)
    ws, scales = _model_ws(m)
    log = []
    _spy(monkeypatch, m, '_pooled_inference', log)
    m.predictions_only = True
    with torch.no_grad(), m.packed_weights():
        monkeypatch.setattr(MODEL, 'POOLED_INFERENCE', False)
        warm = _model_frame(m, pf, of, sf)                     # the message path once, eagerly (no fold is made)
        monkeypatch.setattr(MODEL, 'POOLED_INFERENCE', True)
        torch.cuda.synchronize()
        assert m._ph2 is None and log == []
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = _model_frame(m, pf, of, sf)
        assert m._ph2 is None and len(log) == 1 and log[0][1] is None
        out.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out, warm)
        eager = _model_frame(m, pf, of, sf)                    # outside capture the same block now makes the fold
        assert m._ph2 is not None and log[1][1] is not None
        torch.cuda.synchronize()
    want = ref64(ws, [pf, of], sf, scales, m.tau)[0]
    report('captured frame without a fold (message path)', out, want)
    report('the next eager frame (pooled)', eager, want)
