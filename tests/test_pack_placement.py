"""CPU-only: where a deferred weight pack rides in a split relative-feature forward launch (piml_amd/csrc/reduce.hpp: PackWork,
relfeat.hip: relfeat_go) -- the host rule and the obstacle workgroups' strides, through the library's diagnostic entries (they call
the very functions the kernel and the launcher use; no GPU call is made)."""
import ctypes

import pytest

# pack shapes (nbr, has_head, has_fold, skip_f32): the benchmarked step (plain images, the head's, the folded ones), the message
# path with the head, pinnsf_bm (neither head nor fold)
SUMS, MSGS, BM = (2, 1, 1, 1), (2, 1, 0, 1), (2, 0, 0, 1)
# launches of profiles/r13_pack_placement.md: (waves, obstacle workgroups) the launcher gives them
LAUNCHES = {'n122': (4, 31), 'n488': (4, 122), 'n1024': (8, 128), 'n4096_bench': (16, 256), 'rank_2048x16384': (8, 256)}


def _plan(form, waves, nb, shape):
    from piml_amd import _lib
    blocks, share = ctypes.c_int(-1), ctypes.c_int(-1)
    r = _lib.lib().piml_relfeat_pack_plan(form, waves, nb, *shape, ctypes.byref(blocks), ctypes.byref(share))
    return r, blocks.value, share.value


def test_block_counts_of_the_benchmarked_pack():
    # 1024 threads: two fold groups a block, 3 x 192 groups -> 288 fold blocks; 68 plain blocks; one zero-row block per encoder
    assert _plan(0, 16, 256, SUMS)[1] == 68 + 288 + 2
    # 512 and 256 threads: one fold group a block
    assert _plan(0, 8, 128, SUMS)[1] == _plan(0, 8, 128, MSGS)[1] + 576
    assert _plan(0, 4, 31, SUMS)[1] == _plan(0, 4, 31, MSGS)[1] + 576
    assert _plan(0, 4, 31, MSGS)[1] > 2 * _plan(0, 8, 31, MSGS)[1] - 8      # half the threads: twice the plain blocks


@pytest.mark.parametrize('name, shape, share', [
    # the table of profiles/r13_pack_placement.md: the tail form loses at every one of these, so the default keeps them all on the
    # trailing form; the share is the chain the forced tail form gives one obstacle workgroup
    ('n4096_bench', SUMS, 2),            # 358 blocks over 256 workgroups
    ('rank_2048x16384', SUMS, 3),        # 713 over 256
    ('n1024', SUMS, 6),                  # 713 over 128
    ('n488', SUMS, 7),                   # 848 over 122
    ('n122', SUMS, 28),                  # 848 over 31
    ('n1024', MSGS, 2), ('n122', MSGS, 9), ('n122', BM, 9), ('n4096_bench', BM, 1),
])
def test_default_keeps_the_trailing_form_at_every_shape_of_the_table(name, shape, share):
    from piml_amd import _lib
    waves, nb = LAUNCHES[name]
    default = _lib.lib().piml_relfeat_pack_form(-1)
    assert default == 0
    form, blocks, got = _plan(default, waves, nb, shape)
    assert form == 0 and got == share == -(-blocks // nb)
    assert _plan(1, waves, nb, shape)[0] == 1                                 # forced: the tail form, in any split launch


def test_forms_over_wave_counts_and_row_counts():
    for waves in (4, 8, 16):
        for rows in list(range(1, 70)) + [122, 488, 1000, 1024, 2048, 4096, 5000]:
            nb = -(-rows // waves)
            assert _plan(0, waves, nb, SUMS)[0] == 0 and _plan(1, waves, nb, SUMS)[0] == 1
    assert _plan(0, 5, 10, SUMS)[0] < 0 and _plan(2, 4, 10, SUMS)[0] < 0      # bad arguments
    assert _plan(1, 4, 0, SUMS)[0] == 0                                       # no obstacle workgroups: nothing to ride in


@pytest.mark.parametrize('nb, total', [(1, 7), (2, 848), (3, 358), (31, 848), (128, 713), (256, 358), (256, 65), (400, 358), (7, 0)])
def test_strides_cover_every_pack_block_exactly_once(nb, total):
    from piml_amd import _lib
    L = _lib.lib()
    seen, longest = [], 0
    for b in range(nb):
        out = (ctypes.c_int * (total + 1))()
        n = L.piml_relfeat_pack_tail_blocks(b, nb, total, out, total + 1)
        assert 0 <= n <= total
        blocks = list(out[:n])
        assert blocks == sorted(blocks) and all(0 <= x < total for x in blocks)
        seen += blocks
        longest = max(longest, n)
    assert sorted(seen) == list(range(total))
    assert longest == -(-total // nb)
    assert L.piml_relfeat_pack_tail_blocks(nb, nb, total, None, 0) < 0 and L.piml_relfeat_pack_tail_blocks(0, 0, total, None, 0) < 0


def test_switch_returns_the_previous_value():
    from piml_amd import _lib
    L = _lib.lib()
    old = L.piml_relfeat_pack_form(-1)
    try:
        assert L.piml_relfeat_pack_form(1) == old
        assert L.piml_relfeat_pack_form(7) == 1 and L.piml_relfeat_pack_form(-1) == 1      # out of range: a query
        assert L.piml_relfeat_pack_form(0) == 1
        assert L.piml_relfeat_pack_form(-1) == 0
    finally:
        L.piml_relfeat_pack_form(old)
