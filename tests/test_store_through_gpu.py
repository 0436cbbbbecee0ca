"""GPU: the sums-path step (fused_pinnsf forward + backward, compact rows on, collision head on) is BIT FOR BIT what the commit
named in tests/golden/store_through_parent_bits.json computed, after a change that only moved the form of its stores (the
gradient slots written through: piml_amd/csrc/store.hpp).

The fixture is written by tools/make_store_bits.py on gfx950 (a change that alters arithmetic on purpose regenerates it with that
tool and says so); this file shares the tool's step, so both sides allocate every buffer of the fused network pre-set to a NaN
pattern with 256 bytes of it in front and behind:
  * every recorded tensor (acceleration, head output, g_x of both branches, every weight gradient) and every buffer of the step
    (the sums of both branches, the sign words, the h2 rows, the decoder's saved activations, the slot arrays, ...) has the
    fixture's bits -- including what the kernels leave unwritten (rows behind a partial tile, dead rows of a compact tile);
  * the bands around every buffer still hold the pattern (a store of another width that leaves its buffer lands there);
  * the encoder slot arrays hold the pattern in every slot past the plan's count for the branch, and none in the dW2 field of a
    slot that is counted;
  * d/d(state), summed with float atomics in either build, is held to the 1e-5 bar of tests/test_compact_rows_gpu.py against
    float64 instead.
Scenes (k = 6 / 10 as in the benchmark): mixed97 (a partial last tile, fewer tiles than workgroups), mixed200, all (97 agents,
every one with an obstacle in view), none97 (none has one: every workgroup's share of branch 1 is closed-form), chain (1400
agents: more pedestrian tiles than the 256 workgroups, a slot is the sum of several tiles)."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('make_store_bits', os.path.join(ROOT, 'tools', 'make_store_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.FIXTURE) as _fh:
    WANT = json.load(_fh)
ENC_PART1 = 128 * 128 + 1024 + 2 * 128        # floats of an encoder slot: dW2 | dW1 | db2 | db1 (encoder_bwd5.hip: F5_PART1)


def test_fixture_names_its_commit_and_holds_every_scene():
    assert len(WANT['commit']) == 40 and WANT['arch'] == 'gfx950' and WANT['pattern'] == f'{TOOL.PATTERN:08x}'
    assert set(WANT['scenes']) == set(TOOL.SCENES)
    for name, sc in WANT['scenes'].items():
        assert {'acc', 'coll', 'g_x.ped', 'g_x.obs'} <= set(sc['tensors']) and len(sc['tensors']) > 20 and len(sc['buffers']) > 20, name


@pytest.mark.gpu
@pytest.mark.parametrize('name', TOOL.SCENES)
def test_step_has_the_parent_bits_and_stays_inside_its_buffers(oracle, name):
    T = TOOL._tcr()
    out, G, g_state, ref = TOOL.run_scene(oracle, name)
    want = WANT['scenes'][name]
    bad = G.bands_intact()
    assert not bad, f'{name}: the guard bands of {bad} were written to'
    got = TOOL.scene_bits(out, G)
    assert sorted(got['tensors']) == sorted(want['tensors']), f'{name}: the step returns other tensors than the fixture holds'
    diff = [k for k in want['tensors'] if got['tensors'][k] != want['tensors'][k]]
    assert not diff, f'{name}: bits differ from commit {WANT["commit"][:8]} in {diff}: ' + \
        '; '.join(f'{k} {got["tensors"][k]["head"]} vs {want["tensors"][k]["head"]}' for k in diff[:3])
    assert len(got['buffers']) == len(want['buffers']), f'{name}: {len(got["buffers"])} buffers, the fixture holds {len(want["buffers"])}'
    diff = [(i, b['shape']) for i, (b, w) in enumerate(zip(got['buffers'], want['buffers'])) if b != w]
    assert not diff, f'{name}: buffers (allocation index, shape) differ from commit {WANT["commit"][:8]}: {diff}'
    # the encoder slot arrays: [branch][COMPACT_SLOTS][ENC_PART1]; the plan (the first buffer) counts the workgroups of each branch
    plan = G.body(0).view(-1)
    counts = [int(plan[3]), int(plan[4])]
    slots = [G.body(i) for i in range(len(G.bufs)) if G.bufs[i][1][1:] == (ENC_PART1,)]
    assert len(slots) == 2 and counts[0] + counts[1] == slots[0].shape[0] == slots[1].shape[0], (counts, [s.shape for s in slots])
    for b in range(2):
        assert bool((slots[b][counts[b]:] == TOOL.PATTERN).all()), f'{name}: branch {b}: a slot past the plan\'s {counts[b]} was written to'
        assert not bool((slots[b][:counts[b], :128 * 128] == TOOL.PATTERN).any()), f'{name}: branch {b}: dW2 of a counted slot is not written whole'
    err = T._compare(f'{name}: d/d(state)', g_state, ref['state'])
    print(f'\n{name}: d/d(state) {err:.2e} of its largest float64 magnitude')
    assert err <= T.BAR, f'{name}: d/d(state) differs from float64 by {err:.3e} (bar {T.BAR:.0e})'


@pytest.mark.gpu
def test_eager_captured_and_replayed_twice_agree_bitwise(oracle):
    from piml_amd import ops
    T = TOOL._tcr()
    ref = TOOL.reference(oracle, 'mixed200')
    with T._switches(True):
        step = T._Step(ref)

        def body():
            with ops.deferred_slot_sums():
                step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        eager = step.snapshot()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), step.model.packed_weights():
            body()
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append(step.snapshot())
    for tag, other in (('the second replay', replays[1]), ('the eager step', eager)):
        assert T._bits_equal(replays[0]['acc'], other['acc']) and T._bits_equal(replays[0]['coll'], other['coll']), f'outputs differ from {tag}'
        for k, g in replays[0]['params'].items():
            assert T._bits_equal(g, other['params'][k]), f'gradient of {k} differs from {tag}'
