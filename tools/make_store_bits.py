"""Writes tests/golden/store_through_parent_bits.json: the bits of the sums-path step (fused_pinnsf forward + backward, compact
rows on, collision head on) on the scenes of tests/test_store_through_gpu.py, as THIS build computes them on gfx950.

    python tools/make_store_bits.py [output file]

The fixture pins the step bit for bit across changes that move no arithmetic (store width, cache policy, layout of the code):
run this tool on the build whose results are the yardstick -- the parent commit of such a change -- and commit the file; a change
that alters arithmetic on purpose regenerates it and says so.  The file carries the commit it was made from.

What is recorded, per scene: the acceleration, the collision head's output, the gradient of both feature tensors (g_x), every
weight gradient, and EVERY buffer the fused network allocates for the step (`buffers`: the agents' sums of both branches in their
two parts, the sign words, the h2 rows, the decoder's saved activations, the gradient of the sums, both encoders' and both
decoders' slot arrays, ...), each as shape, sha256 of its bytes and its first four words in hex.  The buffers are allocated
through `guarded()`: every byte is pre-set to a NaN pattern, with 256 bytes of it in front of and behind the buffer, so that what
a kernel leaves unwritten (the rows behind a partial tile, the dead rows of a compact tile, slots no workgroup owns) is part of
the recorded bits and a store outside the buffer shows in the bands.  d/d(state) is not recorded: it is summed with float atomics
(relative-feature backward) and moves from run to run in any build."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'store_through_parent_bits.json')
DEV = 'cuda:0'
PATTERN = 0x7FC0DEAD            # a quiet NaN as float32
GUARD = 64                      # words in front of and behind every buffer = 256 bytes
# name -> the scene of tests/test_compact_rows_gpu.py it is, or (agents, seed, side, absent agents, obstacle points)
SCENES = ('mixed97', 'mixed200', 'all', 'none97', 'chain')


def _tcr():
    import test_compact_rows_gpu as T
    return T


def reference(oracle, name):
    """tests/test_compact_rows_gpu.py's float64 reference of the scene (the upstream gradient and d/d(state) come from it);
    none97: its placeholder branch (10 points far away) under 97 agents -- every workgroup's share of branch 1 is closed-form."""
    T = _tcr()
    if name in T.SCENES:
        return T._reference(oracle, name)
    assert name == 'none97'
    old = T.SCENES
    T.SCENES = dict(old, none97=(97, 8, 14.0, 4, lambda s: T._far(10)))
    try:
        return T._reference(oracle, name)
    finally:
        T.SCENES = old


class Guarded:
    """While `active`, torch.empty(...) of a 4-byte type on the device returns the middle of a larger buffer whose every word is
    PATTERN.  `bufs`: [(whole buffer as int32, shape)] in allocation order."""

    def __init__(self):
        self.bufs, self.active, self._inner = [], False, torch.empty

    def empty(self, *size, **kw):
        dt, dev = kw.get('dtype', torch.float32), kw.get('device')
        if not self.active or dev is None or torch.device(dev).type != 'cuda' or dt not in (torch.float32, torch.int32):
            return self._inner(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        n = int(np.prod(shape)) if shape else 1
        whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=dev)
        self.bufs.append((whole, shape))
        return whole[GUARD:GUARD + n].view(dt).view(shape)

    def inside(self, fn):
        def wrapped(*a, **kw):
            old, self.active = self.active, True
            try:
                return fn(*a, **kw)
            finally:
                self.active = old
        return wrapped

    def bands_intact(self):
        """names of the buffers whose guard bands no longer hold the pattern"""
        bad = []
        for i, (whole, shape) in enumerate(self.bufs):
            if not (bool((whole[:GUARD] == PATTERN).all()) and bool((whole[-GUARD:] == PATTERN).all())):
                bad.append(f'buffer {i} {shape}')
        return bad

    def body(self, i):
        whole, shape = self.bufs[i]
        return whole[GUARD:whole.numel() - GUARD].view(shape)


@contextlib.contextmanager
def guarded():
    """the fused network's forward and its sums-path backward allocate their buffers guarded (nothing else does: the relative-
    feature operator's outputs go on to torch)"""
    from piml_amd import ops
    G = Guarded()
    F = ops._FusedPinnsf
    old_fwd, old_bwd, old_empty = F.forward, F._backward_sums, torch.empty
    F.forward = staticmethod(G.inside(old_fwd))
    F._backward_sums = staticmethod(G.inside(old_bwd))
    torch.empty = G.empty
    try:
        yield G
    finally:
        torch.empty = old_empty
        F.forward, F._backward_sums = staticmethod(old_fwd), staticmethod(old_bwd)


class Step:
    """tests/test_compact_rows_gpu.py's step with the gradients of the two feature tensors kept."""

    def __init__(self, ref):
        T = _tcr()
        sc = ref['scene']
        self.n = ref['n']
        t = lambda a: torch.tensor(a, device=DEV)
        self.state = torch.tensor(np.concatenate([sc[k] for k in ('position', 'velocity', 'acceleration')], -1), device=DEV).requires_grad_(True)
        self.dest, self.v0, self.obstacles = t(sc['destination']), t(sc['desired_speed']), t(sc['obstacles'])
        self.g_up = ref['g_up'].to(DEV)
        self.model = T._model(device=DEV)

    def __call__(self):
        from piml_amd import ops
        self.state.grad = None
        for p in self.model.parameters():
            p.grad = None
        pf, of, sf, _, _ = ops.relative_features_packed_self(self.state, self.dest, self.obstacles, self.v0, 0, self.n, return_index=True)
        pf.retain_grad()
        of.retain_grad()
        res = self.model(pf, of, sf)
        res[0].backward(self.g_up)
        torch.cuda.synchronize()
        out = {'acc': res[0].detach(), 'coll': res[-1].detach(), 'g_x.ped': pf.grad, 'g_x.obs': of.grad}
        for k, p in self.model.named_parameters():
            if p.grad is not None:
                out['d/d(' + k + ')'] = p.grad
        return out, self.state.grad


def run_scene(oracle, name):
    """-> (named tensors, the Guarded of the step, d/d(state), the float64 reference)"""
    T = _tcr()
    ref = reference(oracle, name)
    with T._switches(True), guarded() as G:
        out, g_state = Step(ref)()
    return out, G, g_state, ref


def digest(t):
    w = t.detach().contiguous().view(torch.int32).cpu().numpy().reshape(-1)
    return {'shape': list(t.shape), 'sha256': hashlib.sha256(w.tobytes()).hexdigest(),
            'head': [f'{int(x) & 0xFFFFFFFF:08x}' for x in w[:4]]}


def scene_bits(out, G):
    return {'tensors': {k: digest(v) for k, v in out.items()}, 'buffers': [digest(G.body(i)) for i in range(len(G.bufs))]}


def main():
    from oracle import oracle as O
    O.build()
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    try:
        commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = os.environ.get('PIML_STORE_BITS_COMMIT', 'unknown')
    doc = {'commit': os.environ.get('PIML_STORE_BITS_COMMIT', commit), 'arch': torch.cuda.get_device_properties(0).gcnArchName.split(':')[0],
           'pattern': f'{PATTERN:08x}', 'scenes': {}}
    for name in SCENES:
        out, G, _, _ = run_scene(O, name)
        bad = G.bands_intact()
        assert not bad, f'{name}: guard bands overwritten: {bad}'
        doc['scenes'][name] = scene_bits(out, G)
        print(f'{name}: {len(out)} tensors, {len(G.bufs)} buffers')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print(path)


if __name__ == '__main__':
    main()
