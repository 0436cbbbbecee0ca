"""CPU: the preconditions of test_relfeat_ties_gpu.py.  (1) What each scene of relfeat_tie_scenes.py must CONTAIN -- tie groups at
the k-th slot, groups that span an LDS tile or a sharded block's edge, more in-range sources than a wave's ring holds, a source at
exactly the distance threshold -- checked with the oracle alone at topk = 32, which lists the tie group behind the cut: conditions
on the inputs, not measurements of the kernel.  (2) piml_relfeat_plan, the host rule relfeat_launch itself calls: the table of
forms the GPU tests assert, the launcher's refusals, PIML_RELFEAT_WAVES and the two process-wide latches.  No GPU call is made."""
import os
import subprocess
import sys

import numpy as np
import pytest

import relfeat_tie_scenes as TS
from conftest import REPO


def _lists(oracle, name, **over):
    ref = TS.reference(oracle, name, **dict(TS.KMAX, **over))
    return [x.reshape(-1, x.shape[-1]) for x in ref[3:7]]          # ped_idx, obs_idx, ped_dist, obs_dist: (rows, 32)


def test_hall_has_ties_at_the_cut_across_the_tile_and_across_the_block(oracle):
    k = TS.DEFAULT_GEOM['topk_ped']
    pi, oi, pd, od = _lists(oracle, 'hall')
    N = TS.dims('hall')[1]
    full, tied, group = TS.cut_ties(pi, pd, k)
    tile = TS.spans(pi, group, 0, TS.TILE, N)
    (f0, fc), _, _ = TS.BLOCKS['hall']
    block = TS.spans(pi, group, 0, f0, f0 + fc)[f0:f0 + fc]
    ko = TS.DEFAULT_GEOM['topk_obs']
    ofull, otied, _ = TS.cut_ties(oi, od, ko)
    print(f'\n[tie scenes] hall: {full.sum()} full rows, {tied.sum()} with a tie at the cut, {tile.sum()} tie groups across index '
          f'{TS.TILE}, {block.sum()} rows of block [{f0}, {f0 + fc}) with a lower source in the group; obstacle pass: {ofull.sum()} full, '
          f'{otied.sum()} tied at the cut')
    assert tied.sum() >= 1000 and tile.sum() >= 300 and block.sum() >= 100
    assert otied.sum() >= 300


@pytest.mark.parametrize('name', ['hall_x2', 'edge_4096', 'edge_4097', 'slices', 'many_slices', 'small_600', 'small_1500', 'lattice_9000'])
def test_lattice_cases_have_ties_at_the_cut(oracle, name):
    k = TS.DEFAULT_GEOM['topk_ped']
    pi, oi, pd, od = _lists(oracle, name)
    C, N, M = TS.dims(name)
    full, tied, group = TS.cut_ties(pi, pd, k)
    chunk = TS.spans(pi, group, 0, 64, N) | TS.spans(pi, group, 0, 512, N)       # across a 64-candidate chunk / a 512-group
    print(f'\n[tie scenes] {name}: {full.sum()} full rows of {len(full)}, {tied.sum()} with a tie at the cut, {chunk.sum()} across index 64 or 512')
    assert tied.sum() >= len(full) // 10 and chunk.sum() >= 50
    if name == 'edge_4097':                     # the one source of the second tile is somebody's neighbour
        assert (pi[:, :k] == 4096).any() and np.isfinite(TS.scene(name)['position'][4096, 0])
    if name == 'lattice_9000':
        (f0, fc), _, _ = TS.BLOCKS[name]
        block = TS.spans(pi, group, 0, f0, f0 + fc)[f0:f0 + fc] | TS.spans(pi, group, f0, f0 + fc, N)[f0:f0 + fc]
        print(f'[tie scenes] {name}: {block.sum()} rows of block [{f0}, {f0 + fc}) with a tie group on both sides of a block edge')
        assert block.sum() >= 100


def test_obstacle_tiles_has_ties_across_the_obstacle_tile(oracle):
    ko = TS.DEFAULT_GEOM['topk_obs']
    pi, oi, pd, od = _lists(oracle, 'obstacle_tiles')
    M = TS.dims('obstacle_tiles')[2]
    full, tied, group = TS.cut_ties(oi, od, ko)
    tile = TS.spans(oi, group, 0, TS.TILE, M)
    second = (oi[:, :ko] >= TS.TILE).any(-1)
    print(f'\n[tie scenes] obstacle_tiles: {full.sum()} full rows, {tied.sum()} tied at the cut, {tile.sum()} groups across index {TS.TILE}, '
          f'{second.sum()} rows with a neighbour from the second tile')
    assert tile.sum() >= 20 and second.sum() >= 100


def test_pile_fills_the_ring_in_both_passes(oracle):
    sc = TS.scene('pile')
    N, M = TS.dims('pile')[1:]
    g = TS.geom('pile')
    ref = TS.reference(oracle, 'pile')
    pi, oi, pd, od = [x.reshape(N, -1) for x in ref[3:7]]
    crowd = N - TS.PILE_TAIL
    assert pi[0].tolist() == [0, 2, 4, 6, 8, 10] and pi[1].tolist() == [1, 3, 5, 7, 9, 11]
    for i in range(crowd):                              # the six lowest indices of the row's own parity, all at distance 0
        assert pi[i].tolist() == list(range(i % 2, 12, 2)) and not pd[i].any()
    assert np.array_equal(oi[:crowd], np.tile([0, 1, 2, 4, 5, 6, 8, 9, 10, 12], (crowd, 1)))
    p = sc['position']
    nped = TS.within_cut(p, np.nan_to_num(p, nan=1e9), pd[:, g['topk_ped'] - 1])
    nobs = TS.within_cut(p, sc['obstacles'], od[:, g['topk_obs'] - 1])
    print(f'\n[tie scenes] pile: sources within the final cut-off per row: agents {nped[:crowd].min()} .. {nped[:crowd].max()}, '
          f'obstacle points {nobs[:crowd].min()} .. {nobs[:crowd].max()} (ring: {TS.RING})')
    assert nped[:crowd].min() > TS.RING and nobs[:crowd].min() > TS.RING and M >= 1200
    # the loners see themselves only, the absent rows nothing
    assert np.array_equal(pi[crowd:crowd + 4, 0], np.arange(crowd, crowd + 4)) and (pi[crowd:crowd + 4, 1:] == -1).all()
    assert (pi[crowd + 4:] == -1).all() and (oi[crowd:] == -1).all()
    # sharded block: every saved entry is displaced by a lower index of the same distance
    (f0, fc), _, _ = TS.BLOCKS['pile']
    assert (pi[f0:f0 + fc] < f0).all()


@pytest.mark.parametrize('name', sorted(TS.SCENES))
def test_every_case_has_short_rows_and_absent_rows(oracle, name):
    g = TS.geom(name)
    ref = TS.reference(oracle, name)
    pi = ref[3].reshape(-1, ref[3].shape[-1])
    absent = np.isnan(TS.scene(name)['position'][..., 0]).reshape(-1)
    short = (pi[:, -1] < 0) & ~absent
    print(f'\n[tie scenes] {name}: {absent.sum()} absent focal rows, {short.sum()} present rows with fewer than {g["topk_ped"]} in-view sources')
    assert absent.sum() >= 4 and short.sum() >= 4 and (pi[absent] == -1).all()


@pytest.mark.parametrize('thr', [1.0, 1.5])
def test_hall_has_sources_at_exactly_the_distance_threshold(oracle, thr):
    pi, oi, pd, od = _lists(oracle, 'hall', dist_threshold_ped=thr, dist_threshold_obs=thr)
    at = (pd == np.float32(thr)).any(-1)
    print(f'\n[tie scenes] hall, threshold {thr}: {at.sum()} rows with a neighbour at exactly the threshold')
    assert at.sum() >= 100
    assert not (od == np.float32(thr)).any()     # ((odd^2 + odd^2) / 16 is neither 1 nor 2.25: the agents carry this condition)


@pytest.mark.parametrize('name', ['hall', 'slices', 'pile'])
def test_k_at_its_bound_fills_all_32_slots(oracle, name):
    pi, oi, pd, od = _lists(oracle, name)
    full = int((pi[:, 31] >= 0).sum()), int((oi[:, 31] >= 0).sum())
    print(f'\n[tie scenes] {name}, topk 32: rows with 32 live slots: pedestrians {full[0]}, obstacles {full[1]}')
    assert min(full) >= 100


def test_cosines_sit_on_the_threshold(oracle):
    """sight angle 0: the threshold is cos(0) = 1.0 and only sources exactly ahead are in view -- the lattice has them on the
    axes (cosine exactly 1) and on the diagonals (1 or 1 - 2^-24 ... by the rounding of the normalisations)"""
    ref = TS.reference(oracle, 'small_600', sight_angle_ped=0, sight_angle_obs=0)
    pi = ref[3].reshape(-1, ref[3].shape[-1])
    print(f'\n[tie scenes] small_600, sight angle 0: {(pi[:, 0] >= 0).sum()} rows see a source exactly ahead')
    assert (pi[:, 0] >= 0).sum() >= 100 and (pi[:, 0] < 0).sum() >= 100


# ---- the plan ----
def test_plan_gives_every_case_its_form():
    for name, want in TS.FORMS.items():
        got = TS.plan_of(name)
        print(f'[tie scenes] plan {name} {TS.dims(name)}: waves, resident, split, agent tiles, obstacle tiles = {got[1:]}')
        assert got == (0,) + want, name
    # k at its bound and k = 0 for the pedestrians (no pedestrian pass to split off)
    assert TS.plan_of('hall', **TS.KMAX) == (0,) + TS.FORMS['hall'] and TS.plan_of('slices', **TS.KMAX) == (0,) + TS.FORMS['slices']
    assert TS.plan_of('hall', topk_ped=0)[1:4] == (8, 0, 0) and TS.plan_of('slices', topk_ped=0)[1:4] == (16, 1, 0)
    for name, ((f0, fc), local, remote) in TS.BLOCKS.items():
        assert TS.plan_of(name, part=1, focal_count=fc)[:4] == (0,) + local, name
        assert TS.plan_of(name, part=2, focal_count=fc)[:4] == (0,) + remote, name
        assert TS.plan_of(name, part=1, focal_count=fc)[4] == 1 and TS.plan_of(name, part=2, focal_count=fc)[5] == 0


def test_plan_thresholds():
    P = TS.plan
    assert [P(1, n, 10, n, 6, 10)[1] for n in (1023, 1024, 4095, 4096, 4097, 16383, 16384)] == [4, 8, 8, 16, 8, 8, 8]
    assert [P(4, n, 10, n, 6, 10)[1] for n in (255, 256, 1023, 1024, 4095, 4096)] == [4, 8, 8, 16, 16, 8]
    assert P(1, 4096, 10, 4096, 6, 10, has_pack=1)[1] == 8                       # a pack on board: eight waves for sixteen
    # split: one slice, or up to 4096 rows; resident: unsplit, one agent tile, 1 .. 2048 obstacle points
    assert P(2, 2048, 10, 2048, 6, 10)[2:4] == (0, 1) and P(2, 2049, 10, 2049, 6, 10)[2:4] == (1, 0)
    assert P(2, 4096, 2048, 4096, 6, 10)[2:4] == (1, 0) and P(2, 4096, 2049, 4096, 6, 10)[2:4] == (0, 0)
    assert P(2, 4097, 10, 4097, 6, 10)[2:4] == (0, 0)
    assert P(2, 3000, 0, 3000, 6, 10)[2:6] == (0, 0, 1, 0) and P(2, 3000, 10, 3000, 6, 0)[2:4] == (0, 0)
    assert P(1, 8192, 4097, 8192, 6, 10)[4:6] == (2, 2) and P(1, 8193, 4096, 8193, 6, 10)[4:6] == (3, 1)
    # sharded parts: LOCAL stages the block, REMOTE (counted at focal_begin = 0) the rest; REMOTE has no obstacle pass
    assert P(1, 16384, 2000, 2048, 6, 10, part=1)[1:6] == (8, 0, 1, 1, 1)
    assert P(1, 16384, 2000, 2048, 6, 10, part=2)[1:6] == (8, 0, 0, 4, 0)
    assert P(0, 8, 3, 8, 6, 10) == (0, 0, 0, 0, 0, 0) and P(3, 8, 3, 0, 6, 10) == (0, 0, 0, 0, 0, 0)      # empty: nothing is launched


def test_plan_refuses_what_the_launcher_refuses():
    from piml_amd import _lib
    L = _lib.lib()

    def launcher(C, N, M, fc, kp, ko):        # no buffer is touched: sizes are checked first, and C = 0 / fc = 0 return before the pointers
        return L.piml_relfeat_fwd(None, None, None, None, 2, None, None, C, N, M, 0, fc, kp, ko, 0., 0., 4., 4.,
                                  None, None, None, 2, None, None, None)
    for sizes in ((-1, 8, 3, 8, 6, 10), (1, -1, 3, 0, 6, 10), (1, 8, -1, 8, 6, 10), (1, 8, 3, -1, 6, 10), (1, 8, 3, 9, 6, 10),
                  (1, 8, 3, 8, -1, 10), (1, 8, 3, 8, 6, -1), (1, 8, 3, 8, 33, 10), (1, 8, 3, 8, 6, 33), (0, 8, 3, 8, 33, 10)):
        assert TS.plan(*sizes)[0] == 1 and launcher(*sizes) == 1, sizes
    for sizes in ((0, 8, 3, 8, 6, 10), (1, 8, 3, 0, 6, 10), (0, 0, 0, 0, 32, 32)):
        assert TS.plan(*sizes)[0] == 0 and launcher(*sizes) == 0, sizes
    assert TS.plan(1, 8, 3, 8, 6, 10, part=3)[0] == 1 and TS.plan(1, 8, 3, 8, 6, 10, part=-1)[0] == 1
    assert TS.plan(1, 8, 3, 8, 6, 10, part=2)[0] == 0
    assert L.piml_relfeat_plan(1, 8, 3, 8, 6, 10, 0, 0, None, None, None, None, None) == 0               # every output optional


def test_plan_honours_the_waves_variable(monkeypatch):
    for w in (4, 8, 16):
        monkeypatch.setenv('PIML_RELFEAT_WAVES', str(w))           # read on every call, as the launcher does
        for name, want in TS.FORMS.items():
            assert TS.plan_of(name) == (0, w) + want[1:], (name, w)
    for bad in ('5', '0', '32', 'x'):
        monkeypatch.setenv('PIML_RELFEAT_WAVES', bad)
        assert TS.plan_of('hall')[0] == 1
        assert TS.plan(0, 8, 3, 8, 6, 10)[0] == 0                  # (an empty problem returns before the launcher reads it)
    monkeypatch.delenv('PIML_RELFEAT_WAVES')
    assert TS.plan_of('hall') == (0,) + TS.FORMS['hall']


def test_plan_honours_the_process_wide_latches():
    """PIML_RELFEAT_SPLIT=0 / PIML_RELFEAT_RESIDENT=0 are read once per process: a fresh interpreter, no GPU call."""
    code = ('import sys; sys.path.insert(0, sys.argv[1]); import relfeat_tie_scenes as TS; '
            'print(TS.plan(1, 4500, 2500, 4500, 6, 10)[1:4], TS.plan(8, 600, 130, 600, 6, 10)[1:4])')
    env = dict(os.environ, PIML_RELFEAT_SPLIT='0', PIML_RELFEAT_RESIDENT='0', PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, '-c', code, os.path.join(REPO, 'tests')], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split('\n')[0] == '(8, 0, 0) (16, 0, 0)', out.stdout + out.stderr
