"""CPU: the preconditions of test_rowdec_edges_gpu.py.  The restated dispatch of the row decoder (rowdec_shapes.py) agrees
with the library's own piml_rowdecoder_slots and with the text of the launches; every case has the path, split, slab, slots,
last slab and tiles per wave it was chosen for; and the ReLU guard of the cases' inputs replaces no more rows than its cap."""
import pytest

import rowdec_shapes as SH


def test_constants_are_read_from_the_source():
    assert SH.constant('DEC_SLAB') == SH.TILE              # (decoder.hip asserts it too: the dW chunk is the dX tile)
    assert SH.constant('kRowdecBigTiles') >= 1
    with pytest.raises(ValueError):
        SH.constant('kRowdecNoSuchConstant')


def test_the_grid_literal_is_still_in_the_launches():
    """the forward and the two dX launches each ask rowdec_wg_split for 256 workgroups, and launch that many"""
    assert SH.grid_calls_in_source() == 3
    src = SH.source()
    for kernel in ('rowdec_fwd_x3_kernel', 'rowdec_fwd_big_kernel', 'rowdec_bwd_dx_x3_kernel', 'rowdec_bwd_dx_big_kernel'):
        assert f'hipLaunchKernelGGL({kernel}, dim3({SH.GRID}), dim3({64 * SH.WAVES})' in src, kernel
    assert 'return w < 1 ? 1 : (w > total - 1 ? total - 1 : w);' in src
    assert 'tiles0 + tiles1 > kRowdecBigTiles' in src


def test_slots_agree_with_the_library():
    from piml_amd import _lib
    L = _lib.lib()
    rows = set(SH.LIBRARY_ROWS) | {r for c in SH.CASES.values() for r in c['rows']}
    for r in sorted(rows):
        assert SH.slots(r) == L.piml_rowdecoder_slots(r), r
        assert SH.slots(r) <= SH.SLOT_CAP and SH.slab(r) % SH.constant('DEC_SLAB') == 0
        assert 1 <= SH.last_slab_rows(r) <= SH.slab(r)
    assert L.piml_rowdecoder_slots(0) == 0 and L.piml_rowdecoder_slots(-5) == 0 and SH.slots(0) == 0 and SH.slots(-5) == 0


def test_slab_rule_at_its_edges():
    assert [SH.slab(r) for r in (1, 63, 64, 65, 16383)] == [64] * 5
    assert [SH.slab(r) for r in (16384, 16385, 65535, 65536)] == [256] * 4
    assert SH.slab(65537) == 288 and SH.slab(200000) == 800
    assert [SH.slots(r) for r in (1, 63, 64, 65, 16383, 16384, 16385, 65535, 65536, 65537, 200000)] == \
        [1, 1, 1, 2, 256, 64, 65, 256, 256, 228, 250]
    assert SH.chunks(256) == 8 and SH.chunks(33) == 2 and SH.chunks(1) == 1


def test_split_rule_at_its_clamps():
    assert SH.wg_split((700,)) == 256 and SH.wg_split((1, 1)) == 128
    assert SH.wg_split((1, 32800)) == 1 and SH.wg_split((32800, 1)) == 255
    assert SH.wg_split((65537, 33)) == 255 and SH.wg_split((1, 10 ** 6)) == 1
    assert SH.wg_split((24576, 40960)) == 96            # the reference's rows: 96 + 160 workgroups, one tile per wave
    assert SH.tiles_per_wave((24576, 40960), 0) == 1 and SH.tiles_per_wave((24576, 40960), 1) == 1


@pytest.mark.parametrize('name', sorted(SH.CASES))
def test_case_facts(name):
    c = SH.CASES[name]
    got = SH.facts(c['rows'])
    for key, value in got.items():
        assert c[key] == value, (name, key, value)
    for products in ('x3', 'f32'):
        fwd, dx, dw = SH.paths(c['rows'], products)
        assert ('x3' in fwd or 'big' in fwd) == c['many'] and ('x3' in dx or 'big' in dx) == c['many']
        assert dw == ('rowdec_bwd_dw_x3_kernel' if c['many'] and products == 'x3' else 'rowdec_bwd_dw_lds_kernel')


def test_case_arithmetic():
    """the numbers the cases were chosen by"""
    big = SH.constant('kRowdecBigTiles')
    assert SH.CASES['at_threshold']['tiles'] == big and SH.CASES['over_threshold']['tiles'] == big + 1
    assert SH.CASES['one_branch_over']['tiles'] == big + 1 and 32769 % SH.TILE == 1
    assert not SH.many_rows((16384, 16384)) and SH.many_rows((16384, 16385))
    assert SH.chunks(SH.slab(16384)) == 8                                  # the lds dW kernel's 256-row slab of 8 chunks
    assert SH.chunks(SH.last_slab_rows(33)) == 2 and 33 % SH.TILE == 1      # one slot of two chunks, the second with one row
    # a branch of one row: one workgroup, one busy wave
    for name, b in (('lopsided_first', 0), ('lopsided_second', 1)):
        rows = SH.CASES[name]['rows']
        assert rows[b] == 1 and SH.workgroups(rows, b) == 1 and SH.busy_waves(rows, b) == 1
        assert SH.workgroups(rows, 1 - b) == SH.GRID - 1
    # past_slot_cap: branch 1's two tiles on the eight waves of its one workgroup
    assert SH.workgroups((65537, 33), 1) == 1 and SH.busy_waves((65537, 33), 1) == 2
    # three tiles per wave: 279 waves of the one long branch, 140 of each of the two
    assert SH.tiles((139999,)[0]) - 2 * SH.WAVES * SH.GRID == 279
    assert all(SH.tiles(r) - 2 * SH.WAVES * 128 == 140 for r in (70001, 69999))
    assert all(r % SH.TILE for r in (70001, 69999, 139999))                # ragged last tiles
    # live_subset: either branch alone
    assert SH.many_rows((40000,)) and SH.wg_split((40000,)) == SH.GRID and SH.tiles_per_wave((40000,), 0) == 1
    assert not SH.many_rows((3000,)) and SH.tiles(3000) == 94
    # the bottleneck models' rows at 600 and 2100 agents (6 + 10 neighbours)
    assert not SH.many_rows((600 * 6, 600 * 10)) and SH.many_rows((2100 * 6, 2100 * 10))
    assert SH.tiles(12600) + SH.tiles(21000) == 1051
    # only the long cases leave the row counts test_encoder_gpu.py holds to 1e-5
    for name, c in SH.CASES.items():
        assert (max(c['rows']) > 65536 + 17) == (name in SH.LONG), name


@pytest.mark.parametrize('name', sorted(SH.CASES))
def test_relu_guard_stays_under_its_cap(name):
    branches, ups = SH.make_inputs(name)
    for b, (br, r) in enumerate(zip(branches, SH.CASES[name]['rows'])):
        print(f'\n[rowdec] {name} branch {b}: guard replaced {br["replaced"]} of {r} rows (cap {SH.guard_cap(r)}); '
              f'pred / decoded scale of ' + ', '.join(f'{k} {p:.2f} / {d:.2f}' for k, (p, d) in br['scales'].items()))
        assert br['replaced'] <= SH.guard_cap(r), (name, b, br['replaced'])
        assert br['emb'].shape == (r, 128) and ups[0][b][0].shape == (r, 2) and ups[0][b][1].shape == (r, 64)
        # a last tile / slab compared on its own scale has a scale: not a window of rows that happen to be tiny
        assert all(min(s) >= SH.SCALE_FLOOR for s in br['scales'].values()), (name, b, br['scales'])
