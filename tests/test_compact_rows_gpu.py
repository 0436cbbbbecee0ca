"""GPU: compact rows on the sums path (piml_encoder_branch.nbr_idx / plan, `piml_encoder_compact_rows`): the obstacle branch of
the fused network without its agents that have no obstacle in view, against the dense form (the switch off) and against a
float64 evaluation of the same network on the oracle's features.

One step = relative features (HIP) -> model(pf, of, self_features) -> backward with a random upstream gradient on the
acceleration -> relative-feature backward.  Compared, as tests/test_bench_step_gpu.py does (its helpers are imported): the
acceleration, the collision head's output, the state gradient and every weight gradient, each within 1e-5 of the tensor's
largest float64 magnitude, for BOTH forms.  Agents with a float64 pre-activation next to a ReLU kink carry no upstream
gradient; at most 3 % of the agents may be such (the seeds below are fixed so that the float64 reference stays under it).

Scenes (agents, obstacle points; 6 pedestrian / up to 10 obstacle slots):
  mixed97 / mixed200   a short wall and a few single points: agents with 0, 1 .. 9 and 10 obstacles in view, absent (NaN)
                       agents among them, a number of agents with obstacles that is no multiple of 3 (the agents of a compact
                       tile) and a number without that is no multiple of 32
  all                  an obstacle grid over the whole floor, nobody absent: the list of agents without obstacles is empty
  none_k2 / none_k10   2 / 10 points far away (the placeholder branch of a scene without obstacles): no compact tile at all,
                       branch 1 gets the fewest workgroups and does only the closed-form share
  chain                1400 agents over the grid, a few absent: several compact tiles per workgroup (the requests that run a
                       tile ahead), where every smaller scene has fewer tiles than workgroups
The 4096-agent scene of the benchmark runs compact by default in tests/test_bench_step_gpu.py."""
import numpy as np
import pytest
import torch

from test_bench_step_gpu import BAR, KINK_REL, _bits_equal, _compare

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINK_MAX_FRAC = 0.03


def _floor(n, seed, side, absent):
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 2)) * side
    ang = rng.random(n) * 2 * np.pi
    speed = 0.8 + 0.8 * rng.random(n)
    vel = np.stack((np.cos(ang), np.sin(ang)), 1) * speed[:, None]
    dest = pos + vel * (4 + 4 * rng.random((n, 1)))
    acc = 0.1 * rng.standard_normal((n, 2))
    gone = np.zeros(n, bool)
    gone[rng.choice(n, absent, replace=False)] = True
    pos[gone] = np.nan
    dest[gone] = np.nan
    vel[gone] = 0.0
    acc[gone] = 0.0
    f = lambda x: np.ascontiguousarray(x.astype(np.float32))
    return dict(position=f(pos), velocity=f(vel), acceleration=f(acc), destination=f(dest), desired_speed=f(speed[:, None]))


def _wall(side):
    wall = np.stack((np.full(14, side * 0.5), side * 0.3 + 0.45 * np.arange(14)), 1)
    singles = np.array([[0.15, 0.2], [0.8, 0.15], [0.2, 0.85], [0.85, 0.8], [0.5, 0.05]]) * side
    return np.concatenate((wall, singles)).astype(np.float32)


def _grid(side):
    g = np.arange(-2.0, side + 2.01, 1.0)
    return np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)


def _far(points):
    return (np.array([[1e4, 1e4]]) + np.arange(points)[:, None]).astype(np.float32)


# name -> (agents, seed, side of the floor, absent agents, obstacle points)
SCENES = {
    'mixed97': (97, 8, 14.0, 4, lambda s: _wall(s)),
    'mixed200': (200, 1, 20.0, 7, lambda s: _wall(s)),
    'all': (97, 4, 14.0, 0, lambda s: _grid(s)),
    'none_k2': (300, 9, 24.0, 3, lambda s: _far(2)),
    'none_k10': (200, 11, 20.0, 5, lambda s: _far(10)),
    'chain': (1400, 13, 40.0, 30, lambda s: _grid(s)),
}
_CACHE = {}


def _scene(name):
    n, seed, side, absent, obst = SCENES[name]
    sc = _floor(n, seed, side, absent)
    sc['obstacles'] = obst(side)
    return sc


def _model(dtype=torch.float32, device='cpu'):
    import bench
    import piml_amd.models.model as MODEL
    torch.manual_seed(666)
    model = MODEL.PINNSF_multitask(bench.model_args()).eval()
    model.messages_wanted = False           # the caller reads predictions[0] and the head's output: the sums path
    return model.to(dtype).to(device)


def _reference(oracle, name):
    """float64 on the CPU, once per scene: the oracle's features and indices, the network in float64 on them, the relative-feature
    backward restated at the oracle's indices (tests/test_bench_step_gpu.py: reference_step, here with a random upstream gradient)."""
    if name in _CACHE:
        return _CACHE[name]
    import piml_amd.models.model as MODEL
    import torch.nn as nn
    sc = _scene(name)
    n = sc['position'].shape[0]
    keys = ('position', 'velocity', 'acceleration', 'destination')
    pf, of, df, pi, oi, _, _ = oracle.relfeat_fwd(*[sc[k][None] for k in keys], sc['obstacles'], return_index=True)
    sf = np.concatenate([df[0], np.nan_to_num(sc['velocity']), np.nan_to_num(sc['acceleration']), sc['desired_speed']], -1).astype(np.float32)
    with np.errstate(invalid='ignore'):
        dest_live = ~np.isnan(sc['destination'] - sc['position'])
    model64 = _model(torch.float64)
    near = []

    def hook(_m, _inp, out):
        o = out.detach()
        near.append((o.abs() < KINK_REL * o.abs().mean()).reshape(n, -1).any(-1))
    hooks = []
    for mod in model64.modules():
        if isinstance(mod, MODEL.MLP):
            layers = list(mod.mlp)
            for lin, act in zip(layers[0::2], layers[1::2]):
                if isinstance(act, nn.ReLU):
                    hooks.append(lin.register_forward_hook(hook))
    xs = [torch.from_numpy(a).double().requires_grad_(True) for a in (pf[0], of[0], sf)]
    model64.messages_wanted = True          # (the plain torch path; the flag only chooses what the fused dispatch returns)
    try:
        out = model64(*xs)
    finally:
        for h in hooks:
            h.remove()
    kink = torch.stack(near).any(0)
    g_up = torch.from_numpy(np.random.default_rng(1000 + n).standard_normal((n, 2)).astype(np.float32)).double() * (~kink).double()[:, None]
    out[0].backward(g_up)
    gp, go, gs = [x.grad for x in xs]
    g = torch.zeros(n, 6, dtype=torch.float64)
    focal = torch.arange(n)
    pit = torch.from_numpy(pi[0]).long()
    live = pit >= 0
    g.index_add_(0, pit[live], gp[live])
    g.index_add_(0, focal, -(gp * live[..., None]).sum(1))
    live_o = torch.from_numpy(oi[0]).long() >= 0
    g.index_add_(0, focal, -(go * live_o[..., None]).sum(1))
    own = torch.zeros(n, 6, dtype=torch.float64)
    own[:, 0:2] = -torch.where(torch.from_numpy(dest_live), gs[:, 0:2], torch.zeros_like(gs[:, 0:2]))
    own[:, 2:6] = gs[:, 2:6]
    g.index_add_(0, focal, own)
    ref = dict(scene=sc, n=n, kink=kink, g_up=g_up.float(), acc=out[0].detach(), coll=out[-1].detach(), state=g,
               params={k: p.grad for k, p in model64.named_parameters()}, obs_count=live_o.sum(-1).numpy(), k_obs=oi.shape[-1])
    _CACHE[name] = ref
    return ref


class _Step:
    """The step on the device, eager or captured; `touch`: a torch in-place operation on the obstacle features between the
    feature operator and the model (the features keep their values, the fused network must drop their indices)."""

    def __init__(self, ref, touch=False):
        sc = ref['scene']
        self.n, self.touch = ref['n'], touch
        t = lambda a: torch.tensor(a, device=DEV)
        self.state = torch.tensor(np.concatenate([sc[k] for k in ('position', 'velocity', 'acceleration')], -1), device=DEV).requires_grad_(True)
        self.dest, self.v0, self.obstacles = t(sc['destination']), t(sc['desired_speed']), t(sc['obstacles'])
        self.g_up = ref['g_up'].to(DEV)
        self.model = _model(device=DEV)
        self.out = None

    def __call__(self):
        from piml_amd import ops
        self.state.grad = None
        for p in self.model.parameters():
            p.grad = None
        pf, of, sf, _, _ = ops.relative_features_packed_self(self.state, self.dest, self.obstacles, self.v0, 0, self.n, return_index=True)
        if self.touch:
            of.add_(0.0)
        res = self.model(pf, of, sf)
        res[0].backward(self.g_up)
        self.out = dict(acc=res[0].detach(), coll=res[-1].detach(), state=self.state.grad,
                        params={k: p.grad for k, p in self.model.named_parameters()})
        return self.out

    def snapshot(self):
        torch.cuda.synchronize()
        o = self.out
        return dict(acc=o['acc'].clone(), coll=o['coll'].clone(), state=o['state'].clone(), params={k: (None if v is None else v.clone()) for k, v in o['params'].items()})


class _switches:
    """compact rows on / off, and the sums path for scenes below the few-rows bound of the training kernels."""

    def __init__(self, compact):
        self.compact = compact

    def __enter__(self):
        from piml_amd import _lib
        L = _lib.lib()
        self.old = (L.piml_encoder_compact_rows(1 if self.compact else 0), L.piml_encoder_split_tiles_train(0))

    def __exit__(self, *exc):
        from piml_amd import _lib
        L = _lib.lib()
        L.piml_encoder_compact_rows(self.old[0])
        L.piml_encoder_split_tiles_train(self.old[1])


def _errors(form, snap, ref):
    errs = {'acc': _compare(f'{form}: acceleration', snap['acc'], ref['acc']),
            'collision': _compare(f'{form}: collision output', snap['coll'], ref['coll']),
            'd/d(state)': _compare(f'{form}: d/d(state)', snap['state'], ref['state'])}
    for k, want in ref['params'].items():
        got = snap['params'][k]
        if want is None:
            assert got is None or not bool(got.any()), f'{form}: {k} has a gradient the float64 step does not have'
            continue
        assert got is not None and bool(torch.isfinite(got).all()), f'{form}: gradient of {k} missing or not finite'
        errs[k] = _compare(f'{form}: d/d({k})', got, want)
    worst = max(errs, key=lambda k: errs[k])
    print(f'\n{form}: acc {errs["acc"]:.2e}, collision {errs["collision"]:.2e}, d/d(state) {errs["d/d(state)"]:.2e}, worst {worst} {errs[worst]:.2e}')
    for k, e in errs.items():
        assert e <= BAR, f'{form}: {k} differs from float64 by {e:.3e} of its largest magnitude (bar {BAR:.0e})'
    return errs


_HANDED = [0]       # index tensors fused_pinnsf found for its obstacle features = forwards that ran compact


@pytest.fixture(autouse=True)
def _spy(monkeypatch):
    """fused_pinnsf asks ops._nbr_idx_of only when the switch, the backward form and the shape allow compact rows, and hands the
    library a plan exactly when it answers with an index tensor."""
    from piml_amd import ops
    inner = ops._nbr_idx_of

    def spy(x):
        idx = inner(x)
        _HANDED[0] += idx is not None
        return idx
    monkeypatch.setattr(ops, '_nbr_idx_of', spy)


def _compact_forwards():
    return _HANDED[0]


def test_scenes_hold_the_cases_they_are_meant_to(oracle):
    """On the CPU side: what each scene is in the file for, from the oracle's indices."""
    for name in SCENES:
        ref = _reference(oracle, name)
        cnt, n = ref['obs_count'], ref['n']
        assert float(ref['kink'].float().mean()) <= KINK_MAX_FRAC, f'{name}: {int(ref["kink"].sum())} of {n} agents next to a ReLU kink'
        with_obs, without = int((cnt > 0).sum()), int((cnt == 0).sum())
        absent = np.isnan(ref['scene']['position'][:, 0])
        if name.startswith('mixed'):
            assert set(range(11)) <= set(cnt.tolist()), f'{name}: obstacle counts {sorted(set(cnt.tolist()))}'
            assert with_obs % 3 and without % 32 and absent.any()
            assert (cnt[:-1] > 0).__xor__(cnt[1:] > 0).any()
        elif name == 'all':
            assert without == 0 and ref['k_obs'] == 10
        elif name.startswith('none'):
            assert with_obs == 0 and ref['k_obs'] == (2 if name == 'none_k2' else 10)
        else:
            assert -(-with_obs // 3) + -(-n * 6 // 32) > 2 * 256 and without > 0      # more tiles than two per workgroup


@pytest.mark.parametrize('name', list(SCENES))
def test_step_matches_float64_compact_and_dense(oracle, name):
    ref = _reference(oracle, name)
    snaps = {}
    for compact in (True, False):
        with _switches(compact):
            before = _compact_forwards()
            step = _Step(ref)
            step()
            snaps[compact] = step.snapshot()
            assert _compact_forwards() - before == (1 if compact else 0), f'{name}: the {"compact" if compact else "dense"} form did not run'
        _errors(f'{name} {"compact" if compact else "dense"}', snaps[compact], ref)
    # the two forms against each other: the same bar (a row sits elsewhere in its tile, the zero row's constant is rounded once)
    for key in ('acc', 'coll', 'state'):
        assert _compare(f'{name}: compact vs dense {key}', snaps[True][key], snaps[False][key].double().cpu()) <= BAR
    for k, g in snaps[False]['params'].items():
        if g is not None:
            assert _compare(f'{name}: compact vs dense d/d({k})', snaps[True]['params'][k], g.double().cpu()) <= BAR


@pytest.mark.parametrize('name', ['mixed200', 'none_k10'])
def test_captured_step_replays_bitwise_and_equals_eager(oracle, name):
    from piml_amd import ops
    ref = _reference(oracle, name)
    with _switches(True):
        step = _Step(ref)

        def body():
            with ops.deferred_slot_sums():
                step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        eager = step.snapshot()
        before = _compact_forwards()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), step.model.packed_weights():
            body()
        assert _compact_forwards() - before == 1
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append(step.snapshot())
    _errors(f'{name} replay', replays[0], ref)
    for tag, other in (('the second replay', replays[1]), ('the eager step', eager)):
        assert _bits_equal(replays[0]['acc'], other['acc']) and _bits_equal(replays[0]['coll'], other['coll']), f'{name}: outputs differ from {tag}'
        for k, g in replays[0]['params'].items():
            assert _bits_equal(g, other['params'][k]), f'{name}: gradient of {k} differs from {tag}'


def test_features_modified_in_place_take_the_dense_path(oracle):
    ref = _reference(oracle, 'mixed97')
    with _switches(True):
        before = _compact_forwards()
        step = _Step(ref, touch=True)
        step()
        snap = step.snapshot()
        assert _compact_forwards() == before, 'features written to since the feature operator returned them still ran compact'
    _errors('mixed97 touched', snap, ref)


def test_one_wave_backward_keeps_the_dense_path(oracle):
    """piml_encoder_sums_bwd(1) selects the one-wave backward, which knows no plan: the step must run dense, not fail."""
    from piml_amd import _lib
    ref = _reference(oracle, 'mixed200')
    L = _lib.lib()
    old = L.piml_encoder_sums_bwd(1)
    try:
        with _switches(True):
            before = _compact_forwards()
            step = _Step(ref)
            step()
            snap = step.snapshot()
            assert _compact_forwards() == before, 'compact rows chosen under the one-wave backward'
    finally:
        L.piml_encoder_sums_bwd(old)
    _errors('mixed200 one-wave backward', snap, ref)
