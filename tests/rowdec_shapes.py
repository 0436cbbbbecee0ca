"""Which kernels a call of the row decoder (piml_rowdecoder_fwd / _fwd_packed / _bwd_acc, piml_amd/csrc/decoder.hip) launches
and how it cuts the rows, restated from the host code: the dW slab of a branch (rowdec_slab), its slots
(piml_rowdecoder_slots), the workgroups of branch 0 on the many-rows kernels (rowdec_wg_split), the many-rows predicate and the
tiles a wave of those kernels walks.  DEC_SLAB and kRowdecBigTiles are read out of the source; the literals without a name
(the grid of 256 workgroups, the 16 384-row step of the slab floor, the floors of 64 and 256 rows, the cap of 256 slots) are
restated here and tied down by test_rowdec_shapes.py: `slots` against the library's own piml_rowdecoder_slots, the grid by
the text of the call of rowdec_wg_split.  A retune changes what these functions return, so the preconditions of the cases
(test_rowdec_shapes.py, and again inside test_rowdec_edges_gpu.py before a launch) fail instead of the tests quietly going
back to shapes test_encoder_gpu.py covers already.

Also the inputs of the cases, made on the CPU as test_fused_row_decoder_matches_float64 makes them, with its ReLU guard."""
import functools
import os
import re

import torch

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'piml_amd', 'csrc', 'decoder.hip')


@functools.lru_cache(maxsize=None)
def source():
    with open(SOURCE) as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def constant(name):
    """the value of `constexpr int name = <int>;` in decoder.hip"""
    found = re.findall(r'constexpr\s+int\s+' + re.escape(name) + r'\s*=\s*(\d+)\s*;', source())
    if len(found) != 1:
        raise ValueError(f'{name}: {len(found)} definitions in {SOURCE}')
    return int(found[0])


TILE = 32                   # rows of a dX / forward tile (one wave of the many-rows kernels, one workgroup of the others)
GRID = 256                  # workgroups of the many-rows forward and dX kernels
WAVES = 8                   # waves of one of them: workgroup w of a branch starts at tiles 8 w .. 8 w + 7
SLAB_STEP_ROWS = 16384      # rowdec_slab: below it the floor of a slab is SLAB_FEW rows, from it on SLAB_MANY
SLAB_FEW, SLAB_MANY = 64, 256
SLOT_CAP = 256              # slots of a branch at most: (rows + 255) / 256 rows to a slab before rounding up
GRID_CALL = 'rowdec_wg_split(br, nbr, 256)'
LIBRARY_ROWS = (1, 63, 64, 65, 16383, 16384, 16385, 65535, 65536, 65537, 200000)


def grid_calls_in_source():
    """how often the launches ask rowdec_wg_split for GRID workgroups (the forward once, each of the two dX launches once)"""
    return source().count(GRID_CALL)


def slab(rows):
    s = (rows + SLOT_CAP - 1) // SLOT_CAP
    s = (s + constant('DEC_SLAB') - 1) // constant('DEC_SLAB') * constant('DEC_SLAB')
    return max(s, SLAB_FEW if rows < SLAB_STEP_ROWS else SLAB_MANY)


def slots(rows):
    return 0 if rows <= 0 else -(-rows // slab(rows))


def last_slab_rows(rows):
    return rows - (slots(rows) - 1) * slab(rows)


def chunks(rows_of_a_slab):
    """the DEC_SLAB-row chunks a dW workgroup walks for a slab of that many rows"""
    return -(-rows_of_a_slab // constant('DEC_SLAB'))


def tiles(rows):
    return -(-rows // TILE)


def many_rows(rows):
    """rows: the row counts of the branches of ONE launch"""
    return sum(tiles(r) for r in rows) > constant('kRowdecBigTiles')


def wg_split(rows, total=GRID):
    """workgroups of branch 0 (the C expression: a double product, + 0.5, truncated, then clamped to 1 .. total - 1)"""
    if len(rows) < 2:
        return total
    w = int(total * float(rows[0]) / (float(rows[0]) + float(rows[1])) + 0.5)
    return 1 if w < 1 else (total - 1 if w > total - 1 else w)


def workgroups(rows, b):
    return wg_split(rows) if b == 0 else GRID - wg_split(rows)


def tiles_per_wave(rows, b):
    """the most tiles one wave of branch b walks on the many-rows kernels: tile 8 w + wave, then every 8 * workgroups-th"""
    return -(-tiles(rows[b]) // (WAVES * workgroups(rows, b)))


def busy_waves(rows, b):
    """waves of branch b with at least one tile"""
    return min(tiles(rows[b]), WAVES * workgroups(rows, b))


def paths(rows, products):
    """kernel of the forward, the dX and the dW launch for these branches (products: 'x3' or 'f32')"""
    if not many_rows(rows):
        return ('rowdec_fwd_kernel', 'rowdec_bwd_dx_kernel', 'rowdec_bwd_dw_lds_kernel')
    if products == 'x3':
        return ('rowdec_fwd_x3_kernel', 'rowdec_bwd_dx_x3_kernel', 'rowdec_bwd_dw_x3_kernel')
    return ('rowdec_fwd_big_kernel', 'rowdec_bwd_dx_big_kernel', 'rowdec_bwd_dw_lds_kernel')


def facts(rows):
    """what a case states about its rows, computed from the restated dispatch"""
    many = many_rows(rows)
    return dict(many=many, tiles=sum(tiles(r) for r in rows), split=wg_split(rows) if many and len(rows) > 1 else None,
                slab=tuple(slab(r) for r in rows), slots=tuple(slots(r) for r in rows),
                last_slab=tuple(last_slab_rows(r) for r in rows),
                tiles_per_wave=max(tiles_per_wave(rows, b) for b in range(len(rows))) if many else None)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of test_rowdec_edges_gpu.py with the facts they were chosen for (checked by hand against the constants of today;
# test_rowdec_shapes.py holds `facts(rows)` to them)

CASES = {
    # 1024 tiles: the last launch of one workgroup per tile, a grid of 1024; the lds dW kernel on 256-row slabs of 8 chunks
    'at_threshold': dict(rows=(16384, 16384), seed=21, many=False, tiles=1024, split=None, slab=(256, 256), slots=(64, 64),
                         last_slab=(256, 256), tiles_per_wave=None),
    # 1025 tiles: the first many-rows launch; branch 1 ends in a slab AND a tile of a single row
    'over_threshold': dict(rows=(16384, 16385), seed=22, many=True, tiles=1025, split=128, slab=(256, 256), slots=(64, 65),
                           last_slab=(256, 1), tiles_per_wave=1),
    # the cap of 256 slots from below the 16 384-row step (slabs of 64) and at 65 536 rows (slabs of 256)
    'slot_cap': dict(rows=(16383, 65536), seed=23, many=True, tiles=2560, split=51, slab=(64, 256), slots=(256, 256),
                     last_slab=(63, 256), tiles_per_wave=2),
    # past the cap the slab grows by 32 rows; branch 1 is one slot of two chunks, the second with one row; split clamped to 255
    'past_slot_cap': dict(rows=(65537, 33), seed=24, many=True, tiles=2051, split=255, slab=(288, 64), slots=(228, 1),
                          last_slab=(161, 33), tiles_per_wave=2),
    # a branch of ONE row on one workgroup (split clamped to 1 / to 255): seven of its waves and 31 lanes of the eighth idle
    'lopsided_first': dict(rows=(1, 32800), seed=25, many=True, tiles=1026, split=1, slab=(64, 256), slots=(1, 129),
                           last_slab=(1, 32), tiles_per_wave=1),
    'lopsided_second': dict(rows=(32800, 1), seed=26, many=True, tiles=1026, split=255, slab=(256, 64), slots=(129, 1),
                            last_slab=(32, 1), tiles_per_wave=1),
    'one_branch_small': dict(rows=(700,), seed=27, many=False, tiles=22, split=None, slab=(64,), slots=(11,),
                             last_slab=(60,), tiles_per_wave=None),
    # one branch on all 256 workgroups, the last tile and the last slab of one row
    'one_branch_over': dict(rows=(32769,), seed=28, many=True, tiles=1025, split=None, slab=(256,), slots=(129,),
                            last_slab=(1,), tiles_per_wave=1),
    # 4375 tiles on 2048 waves: 279 waves walk three tiles (the steady state of the x3 dX kernel's row prefetch)
    'one_branch_long': dict(rows=(139999,), seed=29, many=True, tiles=4375, split=None, slab=(576,), slots=(244,),
                            last_slab=(31,), tiles_per_wave=3),
    'two_long': dict(rows=(70001, 69999), seed=30, many=True, tiles=4376, split=128, slab=(288, 288), slots=(244, 244),
                     last_slab=(17, 15), tiles_per_wave=3),
    # forward on the many-rows kernels; a backward of branch 0 alone stays there with one branch, one of branch 1 alone runs
    # 94 tiles on the few-rows kernels (on the h1 / d2 the many-rows forward wrote)
    'live_subset': dict(rows=(40000, 3000), seed=31, many=True, tiles=1344, split=238, slab=(256, 64), slots=(157, 47),
                        last_slab=(64, 56), tiles_per_wave=1),
}
LONG = ('one_branch_long', 'two_long')          # past the 65 553 rows a branch has in test_encoder_gpu.py: the yardstick rule
BOUND = 1e-5                                    # the bound test_encoder_gpu.py holds this operator to, both products modes
GUARD = 1e-5                                    # a float64 pre-activation closer to zero than this: the row gets the zero embedding
SCALE_FLOOR = 0.05                              # max-abs of pred / decoded over a last tile / slab, of the whole tensor's


def guard_cap(rows):
    """rows of a branch the ReLU guard may replace (the expected share is 64 * 2e-5 * phi(0) / 1.19 = 4e-4)"""
    return max(2, int(1e-3 * rows))


def row_windows(rows):
    """the row ranges a row-indexed tensor of a branch is compared on a second time: its last tile and its last dW slab"""
    return {'last tile': (TILE * (tiles(rows) - 1), rows), 'last slab': (slab(rows) * (slots(rows) - 1), rows)}


def make_inputs(name, extra_upstreams=0):
    """CPU tensors of a case, as test_fused_row_decoder_matches_float64 draws them (one generator: per branch the embeddings,
    then the six weights; then the upstream gradients of pred, then those of decoded): per branch `emb`, `ws` (w1 b1 w2 b2 w3
    b3), `replaced` (rows the guard gave the zero embedding) and `scales` (window -> max-abs of float64 pred and decoded over
    the window, of the whole tensor's); `ups` is a list of 1 + extra_upstreams lists of per-branch (g_pred, g_decoded)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c['seed'])
    branches = []
    for r in c['rows']:
        emb = torch.randn(r, 128, generator=g) * 0.7
        ws = [torch.randn(*shp, generator=g) * 0.15 for shp in ((64, 128), (64,), (64, 64), (64,), (2, 64), (2,))]
        # a hidden unit within rounding of zero is on either side of the ReLU's step depending on the summation order: those
        # rows get the zero embedding, whose pre-activation is b1
        w64 = [w.double() for w in ws]
        z = emb.double() @ w64[0].t() + w64[1]
        near = (z.abs() < GUARD).any(1)
        emb[near] = 0.0
        assert float(ws[1].abs().min()) > GUARD
        d = torch.relu(emb.double() @ w64[0].t() + w64[1]) @ w64[2].t() + w64[3]
        p = d @ w64[4].t() + w64[5]
        scales = {k: (float(p[a:b].abs().max() / p.abs().max()), float(d[a:b].abs().max() / d.abs().max()))
                  for k, (a, b) in row_windows(r).items()}
        branches.append(dict(emb=emb, ws=ws, replaced=int(near.sum()), scales=scales))
    ups = []
    for _ in range(1 + extra_upstreams):
        gp = [torch.randn(r, 2, generator=g) for r in c['rows']]
        gd = [torch.randn(r, 64, generator=g) * 0.1 for r in c['rows']]
        ups.append(list(zip(gp, gd)))
    return branches, ups
