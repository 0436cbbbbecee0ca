"""CPU: the group side of the statistics fit without a GPU -- stats_objective's arithmetic on hand-made GroupStats (the four
default terms, speed_ratio_diff at weight 0 and 1, an unknown weight), the search of calibrate_mlapm_to_stats moving Ag
through `evaluate=` inside Ag >= 0, its refusals (Ag without an init value, group_dist without Ag, a scene without groups),
the command line's parser errors, and piml_group_components' argument checks through the library."""
import math
import types

import numpy as np
import pytest

INIT = {'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}
GROUP_KEYS = ('group_fraction_diff', 'size_l1', 'member_distance_l1', 'abreast_l1', 'speed_ratio_diff')


def groups(singles=80, pairs_tracks=20, dist_bin=5, abreast_bin=0, grouped_speed=1.0, link_frames=400, r_bins=20, a_bins=10):
    """one member: `singles` tracks alone and `pairs_tracks` in groups of two, 100 steps each; singles walk 1.0 m/s, the
    grouped tracks `grouped_speed`; every linked pair-frame in one distance bin and one formation bin"""
    from piml_amd.groupstats import G_MAX, Q, GroupStats, make_options
    z = lambda *shape: np.zeros((1,) + shape, np.int64)
    a = {k: z() for k in ('pairs', 'together', 'dist_sum', 'abreast_skipped', 'link_frames', 'candidates', 'links', 'slices')}
    a.update(dist=z(r_bins + 1), abreast=z(a_bins), size_tracks=z(G_MAX + 1), size_path=z(G_MAX + 1), size_steps=z(G_MAX + 1))
    a['size_tracks'][0, 1], a['size_tracks'][0, 2] = singles, pairs_tracks
    a['size_steps'][0, 1], a['size_steps'][0, 2] = 100 * singles, 100 * pairs_tracks
    step = 0.08 * Q                                                    # Q-units of path per step at 1 m/s
    a['size_path'][0, 1], a['size_path'][0, 2] = int(100 * singles * step), int(100 * pairs_tracks * step * grouped_speed)
    a['dist'][0, dist_bin] = a['abreast'][0, abreast_bin] = a['link_frames'][0] = link_frames
    a['links'][0] = a['candidates'][0] = pairs_tracks // 2
    a['slices'][0] = 101
    return GroupStats(a, make_options(0.08, 2.0, 0.5, 0.1, 2.0, 0.8, 0.1, r_bins, a_bins, (0, 101)))


def test_objective_keys_and_default_weights():
    from piml_amd import calibrate as C
    assert C.OBJECTIVE_KEYS['groups'] == GROUP_KEYS
    assert C.DEFAULT_WEIGHTS == {'speed_ratio_diff': 0.0}
    assert C.GROUP_PARAM_NAMES == ('Ag', 'group_dist')
    assert C.DEFAULT_BOUNDS['Ag'] == (0.0, None) and C.DEFAULT_BOUNDS['group_dist'] == (0.0, None)
    assert C.DEFAULT_BOUNDS['tau'] == (1e-3, None) and C.DEFAULT_BOUNDS['Aw'] == (0.0, None)      # the others as they were


def test_stats_objective_group_side():
    from piml_amd.calibrate import stats_objective
    from piml_amd.groupstats import compare_group_stats
    ref = groups()
    J, terms = stats_objective(groups=groups(), ref_groups=ref)
    assert J == 0.0 and set(GROUP_KEYS) <= set(terms)
    # 30 of 100 tracks grouped against 20 of 100: fraction 0.1 apart, sizes |0.7 - 0.8| + |0.3 - 0.2|; the distance and the
    # formation in another bin: 2 each
    sim = groups(singles=70, pairs_tracks=30, dist_bin=9, abreast_bin=4)
    J, terms = stats_objective(groups=sim, ref_groups=ref)
    want = compare_group_stats(sim, ref, 50)
    assert set(terms) == set(want) and all(terms[k] == want[k] for k in GROUP_KEYS[:4])
    assert terms['group_fraction_diff'] == pytest.approx(0.1, abs=1e-12) and terms['size_l1'] == pytest.approx(0.2, abs=1e-12)
    assert terms['member_distance_l1'] == 2.0 and terms['abreast_l1'] == 2.0
    assert math.isnan(terms['speed_ratio_diff'])                     # 20 / 30 grouped tracks < min_count 50 ...
    assert J == pytest.approx(0.1 + 0.2 + 2.0 + 2.0, abs=1e-12)      # ... and at weight 0 it leaves J finite: the four terms
    J1, _ = stats_objective(groups=sim, ref_groups=ref, weights={'speed_ratio_diff': 1.0})
    assert J1 == float('inf')
    # with enough grouped tracks on both sides the term is a number, and the weight switches it on
    big_ref, big = groups(60, 60), groups(60, 60, grouped_speed=0.75)
    J0, t0 = stats_objective(groups=big, ref_groups=big_ref)
    J2, t2 = stats_objective(groups=big, ref_groups=big_ref, weights={'speed_ratio_diff': 2.0})
    assert t0['speed_ratio_diff'] == pytest.approx(0.25, abs=1e-6) and J0 == 0.0
    assert J2 == pytest.approx(0.5, abs=2e-6)
    Jw, _ = stats_objective(groups=sim, ref_groups=ref, weights={'size_l1': 0.0, 'abreast_l1': 0.5})
    assert Jw == pytest.approx(0.1 + 2.0 + 1.0, abs=1e-12)
    with pytest.raises(ValueError, match='unknown'):
        stats_objective(groups=sim, ref_groups=ref, weights={'group_size_l1': 1.0})
    with pytest.raises(ValueError, match='group'):                   # one half of a side is no side
        stats_objective(groups=sim)
    # next to another side: the sum of both
    from test_calibrate_stats import crowd
    Jc, _ = stats_objective(crowd=crowd(1.25), ref_crowd=crowd(1.0))
    Jb, tb = stats_objective(crowd(1.25), None, crowd(1.0), None, None, 50, None, None, sim, ref)
    assert Jb == pytest.approx(Jc + J, abs=1e-12) and 'fd_distance' in tb and 'size_l1' in tb


def search(evaluate, fit=('Ag',), init=None, log=None, **kw):
    from piml_amd.calibrate import calibrate_mlapm_to_stats

    def ev(cands):
        if log is not None:
            log.append([dict(c) for c in cands])
        return evaluate(cands)
    kw = {'population': 8, 'generations': 8, **kw}
    return calibrate_mlapm_to_stats(None, None, version='GC', init={**INIT, 'Ag': 1.0} if init is None else init, fit=fit,
                                    evaluate=ev, **kw)


def test_search_moves_the_group_term_inside_its_bounds():
    from piml_amd.models.mlapm import DEFAULT_GROUP_DIST
    log = []
    res = search(lambda cs: [(c['Ag'] - 3.0) ** 2 for c in cs], log=log, sigma=1.0)
    assert abs(res.params['Ag'] - 3.0) < abs(1.0 - 3.0) and res.final_loss < res.initial_loss == 4.0
    assert all(y <= x for x, y in zip(res.history, res.history[1:]))
    assert res.params['group_dist'] == DEFAULT_GROUP_DIST and res.fit == ('Ag',)
    for g in log:
        for c in g:
            assert c['group_dist'] == DEFAULT_GROUP_DIST and c['version'] == 'GC' and 'Aw' not in c
            assert {k: c[k] for k in INIT} == INIT
    # the optimum lies below the bound: the search walks into Ag = 0 and never past it
    log = []
    res = search(lambda cs: [(c['Ag'] + 2.0) ** 2 + (c['group_dist'] - 1.0) ** 2 for c in cs], fit=('Ag', 'group_dist'),
                 init={**INIT, 'Ag': 1.0, 'group_dist': 0.25}, log=log, sigma=2.0)
    ags = [c['Ag'] for g in log for c in g]
    dists = [c['group_dist'] for g in log for c in g]
    assert min(ags) == 0.0 and min(dists) >= 0.0 and res.params['Ag'] >= 0.0
    assert res.params['group_dist'] != 0.25
    # a fit of the pair law alone carries a group term in init through untouched
    res = search(lambda cs: [(c['A'] - 3.0) ** 2 for c in cs], fit=('A',), init={**INIT, 'Ag': 2.5})
    assert res.params['Ag'] == 2.5 and res.params['group_dist'] == DEFAULT_GROUP_DIST and res.params['A'] != INIT['A']
    # and without one, nothing of it appears
    res = search(lambda cs: [(c['A'] - 3.0) ** 2 for c in cs], fit=('A',), init=dict(INIT))
    assert 'Ag' not in res.params and 'group_dist' not in res.params


def test_group_term_refusals():
    from piml_amd.calibrate import calibrate_mlapm_to_stats
    ev = lambda cs: [0.0] * len(cs)                                  # noqa: E731
    with pytest.raises(ValueError, match='group term has no default'):
        calibrate_mlapm_to_stats(None, None, init=dict(INIT), fit=('Ag',), evaluate=ev)
    with pytest.raises(ValueError, match='group term has no default'):
        calibrate_mlapm_to_stats(None, None, init=dict(INIT), fit=('group_dist',), evaluate=ev)
    with pytest.raises(ValueError, match='group term has no default'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'group_dist': 0.5}, fit=('A',), evaluate=ev)
    with pytest.raises(ValueError, match='Ag >= 0'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'Ag': -1.0}, fit=('A',), evaluate=ev)
    with pytest.raises(ValueError, match='names of'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'Ag': 1.0}, fit=('Ag', 'gaze'), evaluate=ev)
    with pytest.raises(ValueError, match='bounds for unknown'):
        calibrate_mlapm_to_stats(None, None, init={**INIT, 'Ag': 1.0}, fit=('Ag',), evaluate=ev, bounds={'gaze': (0, 1)})
    # a scene that is not a grouped clip scene: refused before anything is launched (no GPU is touched here)
    for law in ('clip', 'gc'):
        with pytest.raises(ValueError, match='the scene has no groups'):
            calibrate_mlapm_to_stats(types.SimpleNamespace(spawn_law=law), (None, None, None, groups()),
                                     init={**INIT, 'Ag': 1.0}, fit=('Ag',))


def test_command_line_refusals(capsys):
    from piml_amd import calibrate as C
    ok = ['--data', 'clip.npy', '--match-stats', '--scene-groups', 'auto', '--fit', 'Ag,group_dist', '--init', 'Ag=3']
    a = C.get_args(ok)
    assert a.fit == ('Ag', 'group_dist') and a.init == {'Ag': 3.0} and a.scene_groups == 'auto'
    assert a.match == ('crowd', 'pairs', 'groups')                   # on by default with a group term
    a = C.get_args(ok + ['--match', 'groups'])
    assert a.match == ('groups',)
    a = C.get_args(['--data', 'clip.npy', '--match-stats', '--scene-groups', 'auto', '--match', 'crowd,groups'])
    assert a.match == ('crowd', 'groups') and a.fit == C.PARAM_NAMES  # the group statistics may be matched without a group term
    assert C.get_args(['--data', 'clip.npy', '--match-stats']).match == ('crowd', 'pairs')       # as before
    for argv, word in ((['--data', 'clip.npy', '--fit', 'Ag', '--init', 'Ag=3'], 'fitted by --match-stats only'),
                       (['--data', 'clip.npy', '--init', 'group_dist=0.5'], 'fitted by --match-stats only'),
                       (['--data', 'clip.npy', '--match-stats', '--scene-groups', 'auto', '--fit', 'Ag'], 'has no default'),
                       (['--data', 'clip.npy', '--match-stats', '--scene-groups', 'auto', '--init', 'group_dist=0.5'],
                        'has no default'),
                       (['--data', 'clip.npy', '--match-stats', '--fit', 'Ag', '--init', 'Ag=3'], '--scene-groups'),
                       (['--data', 'clip.npy', '--scene-groups', 'auto'], '--match-stats'),
                       (ok + ['--match', 'crowd,gaze'], '--match'),
                       (ok[:4] + ['/nonexistent/groups.json'] + ok[5:], '--scene-groups'),
                       (['--data', 'clip.npy', '--match-stats', '--fit', 'gaze'], '--fit'),
                       (['--data', 'clip.npy', '--match-stats', '--init', 'gaze=1'], '--init')):
        with pytest.raises(SystemExit) as ex:
            C.get_args(argv)
        assert ex.value.code == 2, argv
        assert word in capsys.readouterr().err, argv


def _components(L, S=1, N=8, cap=4, min_frames=2, share_q=819, g_max=8, edges=None):
    return L.piml_group_components(edges, None, None, None, S, N, cap, min_frames, share_q, g_max, *([None] * 8), None)


def test_entry_refuses_bad_arguments_without_gpu():
    import ctypes
    from piml_amd import _lib, ops_metrics
    from test_abi import declared_symbols
    assert 'piml_group_components' in set(declared_symbols(('piml_hip.h',))) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES['piml_group_components']) == 19 and ops_metrics.GROUP_MAX_G == 64
    L = _lib.lib()
    for kw in (dict(S=-1), dict(N=-1), dict(cap=-1), dict(N=65537), dict(g_max=0), dict(g_max=65), dict(min_frames=0),
               dict(share_q=0), dict(share_q=1025), dict(share_q=-5)):
        assert _components(L, **kw) == 1, kw
    assert _components(L) == 1                                       # NULL pointers where there is work
    assert _components(L, cap=0) == 1                                # ... also without rows: the outputs are still needed
    for kw in (dict(S=0), dict(N=0), dict(S=0, N=0, cap=0)):         # nothing to do, nothing launched
        assert _components(L, **kw) == 0, kw
    assert _components(L, S=0, g_max=0) == 1                         # the values are checked first
    # every pointer but `edges` given: still refused while cap > 0, before any launch
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.addressof(buf)
    assert L.piml_group_components(None, p, p, p, 1, 8, 4, 2, 819, 8, *([p] * 8), None) == 1


def test_operator_refuses_cpu_tensors_and_wrong_types():
    import torch
    from piml_amd import _lib, ops_metrics
    from piml_amd.groupstats import group_stats
    e, n = torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    st = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.group_components_frames(e, n, st, st, 2, 819)
    with pytest.raises(_lib.PimlHipError):
        ops_metrics.group_stats_frames(torch.zeros(1, 3, 4, 2), torch.ones(1, 3, 4), 0.08, components='device')
    with pytest.raises(ValueError, match='components'):
        ops_metrics.group_stats_frames(torch.zeros(1, 3, 4, 2), torch.ones(1, 3, 4), 0.08, components='gpu')
    with pytest.raises(ValueError, match='components'):
        group_stats(np.zeros((1, 3, 4, 2), np.float32), np.ones((1, 3, 4), np.float32), components='gpu')
