"""CPU: collective-motion statistics (piml_amd.flowstats) without a GPU -- the numpy restatement (flowstats_ref.py) on
hand-counted placements, option validation, axis='auto', the derived quantities on synthetic counts, pooling, merging, JSON,
compare_flow_stats, the command lines' parsing, and the C entry's exports and argument checks (refused before any HIP
call)."""
import math

import numpy as np
import pytest

import flowstats_ref as REF

Q = REF.Q


def _one_frame(P, V, M=None, **kw):
    P = np.asarray(P, np.float32)[None]
    V = np.asarray(V, np.float32)[None]
    M = np.ones(P.shape[:2], np.float32) if M is None else np.asarray(M, np.float32)[None]
    return REF.flow_stats(P, V, M, **kw)


def test_two_perfect_opposite_lanes():
    """two files of 5 along x, 1.03 m between neighbours, 2.04 m apart: farther than lane_width"""
    n = 5
    P = [[1.03 * k, 0.0] for k in range(n)] + [[1.03 * k, 2.04] for k in range(n)]
    V = [[1.2, 0.0]] * n + [[-1.2, 0.0]] * n
    st = _one_frame(P, V)
    assert st['n_ambiguous'] == 0
    assert st['lane_n'].tolist() == [[2 * n]] and st['lane_sum'].tolist() == [[2 * n * Q]] and st['lane_opp'].tolist() == [[0]]
    assert st['lane_same'].tolist() == [[2 * n * (n - 1)]]          # 4 x 1.03 m < lane_length: the whole file
    assert st['dir_plus'].tolist() == [[n]] and st['dir_minus'].tolist() == [[n]]
    within = np.zeros(60, np.int64)
    for i in range(n):
        for j in range(n):
            if i != j:
                within[int(1.03 * abs(i - j) / 0.1)] += 2
    across = st['corr_pairs'][0] - within
    assert (across >= 0).all() and across.sum() == 2 * n * n and st['corr_pairs'][0].sum() == 2 * n * (n - 1) + 2 * n * n
    assert np.array_equal(st['corr_sum'][0], Q * (within - across))       # C = +1 within a lane, -1 across
    for k in REF.OUTPUTS[:8]:
        assert np.array_equal(st['f32'][k], st[k]), k
    assert st['map_n'] is None


def test_alternating_file_lone_agent_and_who_counts():
    # strictly alternating directions in one file along x, 0.83 m apart, lane_length 2: neighbours at 0.83 and 1.66 m
    m = 7
    P = [[0.83 * k, 1.0] for k in range(m)]
    V = [[1.0 if k % 2 == 0 else -1.0, 0.0] for k in range(m)]
    st = _one_frame(P, V, lane_length=2.0)
    ns = [sum(1 for j in range(m) if abs(j - i) == 2) for i in range(m)]
    no = [sum(1 for j in range(m) if abs(j - i) == 1) for i in range(m)]
    assert st['lane_same'].tolist() == [[sum(ns)]] and st['lane_opp'].tolist() == [[sum(no)]] and st['lane_n'].tolist() == [[m]]
    phi = sum(int(np.rint(((a - b) / (a + b)) ** 2 * Q)) for a, b in zip(ns, no))
    assert st['lane_sum'].tolist() == [[phi]] and st['dir_plus'].tolist() == [[4]] and st['dir_minus'].tolist() == [[3]]
    # a lone agent: no band, no pair
    st = _one_frame([[1.0, 1.0]], [[1.0, 0.0]], box=(0.0, 2.0, 0.0, 2.0))
    assert st['lane_n'].sum() == 0 and st['corr_pairs'].sum() == 0 and st['dir_plus'].tolist() == [[1]]
    assert st['map_n'].shape == (1, 4, 4) and st['map_n'][0, 2, 2] == 1 and st['map_vx'][0, 2, 2] == Q and st['map_n'].sum() == 1
    # who counts: mask 0.5, NaN position, a velocity component >= 1024, inf velocity are out; a slow agent is no mover and
    # no lane mover but counts in the map; an agent walking across the axis is a mover but no lane mover
    P = [[0.2, 0.2], [0.7, 0.2], [1.2, 0.2], [1.7, 0.2], [0.2, 1.2], [0.7, 1.2], [1.2, 1.2], [np.nan, 0.2]]
    V = [[1, 0], [1, 0], [1024, 0], [np.inf, 0], [0.05, 0.0], [0, 1], [1, 0], [1, 0]]
    M = [1, 0.5, 1, 1, 1, 1, 1, 1]
    st = _one_frame(P, V, M, box=(0.0, 2.0, 0.0, 2.0))
    assert st['map_n'].sum() == 4                                 # slots 0, 4, 5, 6
    assert st['dir_plus'].tolist() == [[2]] and st['dir_minus'].tolist() == [[0]]         # slots 0 and 6
    assert st['corr_pairs'].sum() == 6                            # movers 0, 5, 6: ordered pairs
    assert st['corr_sum'].sum() == 2 * Q                          # 0-6 parallel (+1 twice), 5 perpendicular to both
    assert st['lane_n'].tolist() == [[0]]                         # 0 and 6 are 1 m apart across the axis: no band
    # the box restricts the focal side only; n_active and frames restrict the sweep
    st = _one_frame([[0.5, 0.5], [1.5, 0.5]], [[1, 0], [1, 0]], box=(0.0, 1.0, 0.0, 1.0))
    assert st['corr_pairs'].sum() == 1 and st['lane_same'].tolist() == [[1]] and st['map_n'].sum() == 1
    st = _one_frame([[0.5, 0.5], [1.5, 0.5]], [[1, 0], [1, 0]], n_active=[1])
    assert st['corr_pairs'].sum() == 0 and st['dir_plus'].tolist() == [[1]]
    P3 = np.zeros((1, 3, 2, 2), np.float32)
    P3[0, :, 1, 0] = 1.0
    st = REF.flow_stats(P3, np.ones_like(P3), np.ones((1, 3, 2), np.float32), frames=(1, 3), axis=(0.0, 1.0))
    assert st['lane_n'].shape == (1, 2) and st['corr_pairs'].sum() == 4 and st['lane_n'].sum() == 0
    # r_max below the bins
    st = _one_frame([[0, 0], [2.55, 0]], [[1, 0], [1, 0]], r_max=2.0)
    assert st['corr_pairs'].sum() == 0 and st['lane_same'].tolist() == [[2]]


def test_ambiguity_is_flagged():
    st = _one_frame([[0, 0], [1.0, 0]], [[1, 0], [1, 0]])                 # r on the edge of bin 10
    assert st['n_ambiguous'] == 2 and st['tol']['corr_pairs'][0, 9:11].tolist() == [2, 2]
    st = _one_frame([[0, 0], [1.05, 0.5]], [[1, 0], [-1, 0]])             # across the axis exactly lane_width
    assert st['n_ambiguous'] >= 2 and st['tol']['lane_n'].tolist() == [[2]]
    st = _one_frame([[0, 0], [1.05, 0.2]], [[0.1, 0], [1, 0]])            # speed exactly v_min
    assert st['n_ambiguous'] >= 2 and st['tol']['dir_plus'].tolist() == [[1]]


def test_check_options_and_axis():
    from piml_amd.flowstats import check_options, parse_axis
    r_max, axis, box, grid, frames = check_options(box=(5, 25, 15, 35), frames=(2, 9), T=10)
    assert r_max == pytest.approx(6.0, rel=1e-6) and axis == (1.0, 0.0) and grid == (40, 40) and frames == (2, 9)
    assert check_options(r_max=2.5)[0] == 2.5 and check_options(axis='auto')[1] == 'auto'
    assert parse_axis('y') == (0.0, 1.0) and parse_axis((3.0, 4.0)) == (float(np.float32(0.6)), float(np.float32(0.8)))
    assert parse_axis(30) == pytest.approx((math.cos(math.pi / 6), 0.5), rel=1e-6) and parse_axis('90')[1] == 1.0
    assert parse_axis('0.6,0.8') == parse_axis([0.6, 0.8])
    for bad in (dict(v_min=0), dict(v_min=float('nan')), dict(r_bin=-1), dict(r_bins=0), dict(r_bins=257), dict(r_bins=2.5),
                dict(r_max=0), dict(r_max=6.5), dict(axis='z'), dict(axis=(0, 0)), dict(axis=(1, 2, 3)),
                dict(axis=float('inf')), dict(lane_width=0), dict(lane_length=-2), dict(cell=0), dict(box=(0, 0, 0, 1)),
                dict(box=(0, 1, 2)), dict(frames=(3, 3)), dict(frames=(0, 11), T=10)):
        with pytest.raises(ValueError):
            check_options(**bad)


def test_auto_axis_of_a_known_direction():
    from piml_amd.flowstats import auto_axis
    rng = np.random.default_rng(3)
    T, N = 6, 40
    ang = math.radians(25.0)
    along = rng.normal(0, 1.2, (T, N, 1)) * np.array([math.cos(ang), math.sin(ang)])
    V = (along + rng.normal(0, 0.05, (T, N, 2))).astype(np.float32)              # both ways along 25 degrees
    P = rng.random((T, N, 2)).astype(np.float32)
    M = np.ones((T, N), np.float32)
    ex, ey = auto_axis(P, V, M)
    assert ex > 0 and math.degrees(math.atan2(ey, ex)) == pytest.approx(25.0, abs=1.0)
    assert abs(ex * ex + ey * ey - 1) < 1e-6
    V2, M2, P2 = V.copy(), M.copy(), P.copy()
    V2[0, :10] = [0.0, 900.0]                  # absent, non-finite and too fast agents do not vote
    M2[0, :5] = 0.0
    P2[0, 5:10, 0] = np.nan
    V2[1, :4] = [0.0, 5000.0]
    V2[2, 0, 0] = np.nan
    got = auto_axis(P2, V2, M2)
    assert math.degrees(math.atan2(got[1], got[0])) == pytest.approx(25.0, abs=1.0)
    assert auto_axis(P[None], V[None], M[None], n_active=[N]) == (ex, ey)
    assert auto_axis(P, np.zeros_like(V), M) == (1.0, 0.0)
    e = auto_axis(P, np.stack([np.zeros((T, N)), np.ones((T, N))], -1).astype(np.float32), M)
    assert e[1] == 1.0 and abs(e[0]) < 1e-7          # straight up: e_y > 0


def _synthetic():
    from piml_amd.flowstats import FlowStats
    rng = np.random.default_rng(0)
    S, Tp, RB, gy, gx = 3, 5, 8, 2, 3
    pairs = rng.integers(60, 200, (S, RB))
    c = np.array([0.9, 0.7, 0.5, 0.3, 0.1, 0.0, -0.1, 0.05])
    arrays = dict(corr_pairs=pairs, corr_sum=np.rint(pairs * c * Q).astype(np.int64), lane_n=rng.integers(1, 9, (S, Tp)),
                  lane_same=rng.integers(20, 40, (S, Tp)), lane_opp=rng.integers(1, 20, (S, Tp)),
                  dir_plus=rng.integers(3, 9, (S, Tp)), dir_minus=rng.integers(1, 5, (S, Tp)),
                  map_n=rng.integers(0, 9, (S, gy, gx)), map_vx=rng.integers(-5 * Q, 5 * Q, (S, gy, gx)),
                  map_vy=rng.integers(-5 * Q, 5 * Q, (S, gy, gx)), slices=np.full(S, Tp))
    arrays['lane_sum'] = arrays['lane_n'] * (Q // 4)
    opts = dict(v_min=0.1, r_bin=0.5, r_bins=RB, r_max=4.0, axis=(1.0, 0.0), lane_width=0.5, lane_length=5.0, cell=0.5,
                box=(0.0, 1.5, 0.0, 1.0), frames=(0, Tp))
    return FlowStats(arrays, opts), arrays, opts


def test_derived_quantities_pooling_json_and_compare(tmp_path):
    from piml_amd.flowstats import FlowStats, compare_flow_stats, merge
    st, arrays, opts = _synthetic()
    assert st.members == 3 and st.pooled().members == 1 and st.member(1).corr_pairs.shape == (1, 8)
    assert np.array_equal(st.pooled().lane_n[0], arrays['lane_n'].sum(0))
    assert np.array_equal(st.select([2, 0]).corr_sum, arrays['corr_sum'][[2, 0]])
    with pytest.raises(IndexError):
        st.select([3])
    c = st.velocity_correlation()
    assert c == pytest.approx([0.9, 0.7, 0.5, 0.3, 0.1, 0.0, -0.1, 0.05], abs=1e-4)
    assert np.isnan(st.velocity_correlation(min_count=10 ** 6)).all()
    # 1/e lies between bins 2 (0.5 at 1.25 m) and 3 (0.3 at 1.75 m)
    assert st.correlation_length() == pytest.approx(1.25 + (0.5 - 1 / math.e) / 0.2 * 0.5, abs=2e-3)
    assert math.isnan(st.correlation_length(min_count=10 ** 6))
    series, mean = st.lane_order()
    assert series.shape == (5,) and series == pytest.approx(0.25) and mean == pytest.approx(0.25)
    same, opp = arrays['lane_same'].sum(), arrays['lane_opp'].sum()
    assert st.same_direction_fraction() == pytest.approx(same / (same + opp))
    a, b = arrays['dir_plus'].sum(), arrays['dir_minus'].sum()
    assert st.chance_same_fraction() == pytest.approx((a * a + b * b) / (a + b) ** 2)
    u, J = st.mean_velocity_field(), st.flow_field()
    n = arrays['map_n'].sum(0)
    assert u.shape == (2, 3, 2) and J.shape == (2, 3, 2) and np.isnan(u[n == 0]).all()
    assert J[..., 0] == pytest.approx(arrays['map_vx'].sum(0) / (Q * 15 * 0.25))
    ok = n > 0
    assert (u[ok] * (n[ok] / (15 * 0.25))[:, None]) == pytest.approx(J[ok])              # J = rho u
    # JSON
    back = FlowStats.from_json(st.to_json(str(tmp_path / 'f.json')))
    again = FlowStats.from_json(str(tmp_path / 'f.json'))
    for k in ('corr_pairs', 'corr_sum', 'lane_n', 'lane_sum', 'map_vx', 'slices'):
        assert np.array_equal(getattr(back, k), getattr(st, k)) and np.array_equal(getattr(again, k), getattr(st, k)), k
    assert back.options == st.options
    with pytest.raises(ValueError):
        FlowStats.from_json({'version': 99})
    nomap = FlowStats({**arrays, 'map_n': None, 'map_vx': None, 'map_vy': None}, {**opts, 'box': None})
    assert FlowStats.from_json(nomap.to_json()).map_n is None and nomap.flow_field() is None
    # compare
    c = compare_flow_stats(st, back)
    assert c['corr_max_diff'] == 0 and c['corr_bins'] == 8 and c['correlation_length_diff'] == 0 \
        and c['lane_order_diff'] == 0 and c['excess_same_fraction_diff'] == 0 and c['flow_distance'] == 0
    assert compare_flow_stats(st, nomap)['flow_distance'] is None
    c2 = compare_flow_stats(st.member(0), st.member(1), min_count=1)
    assert c2['corr_max_diff'] > 0 and 0 < c2['flow_distance'] <= 2
    for k, v in (('r_bin', 0.25), ('axis', (0.0, 1.0)), ('lane_width', 0.6), ('v_min', 0.2)):
        with pytest.raises(ValueError):
            compare_flow_stats(st, FlowStats(arrays, {**opts, k: v}))
    # merge: series end to end, the rest added
    mg = merge([st, st.member(0)])
    assert mg.lane_n.shape == (1, 10) and mg.options['frames'] == (0, 5)
    assert np.array_equal(mg.corr_pairs[0], arrays['corr_pairs'].sum(0) + arrays['corr_pairs'][0])
    assert mg.slices.tolist() == [20] and FlowStats.merge([st]).lane_n.shape == (1, 5)
    with pytest.raises(ValueError):
        merge([st, FlowStats(arrays, {**opts, 'lane_length': 4.0})])


def test_cli_parsing():
    from piml_amd import flowstats, simulate
    a = flowstats.get_args(['--data', 'a.npy', 'b.npy', '--ref', 'r.npy', '--box', 'auto', '--frames', '3:400', '--axis',
                            'auto', '--r_max', '4', '--out', 'o.json'])
    assert a.data == ['a.npy', 'b.npy'] and a.ref == 'r.npy' and a.box == 'auto' and a.frames == (3, 400)
    assert a.axis == 'auto' and a.r_max == 4.0 and a.r_bins == 60 and a.out == 'o.json'
    d = flowstats.get_args(['--data', 'a.npy', '--box', '5,25,15,35', '--axis', '90'])
    assert d.box == (5.0, 25.0, 15.0, 35.0) and d.axis[1] == 1.0 and d.frames is None
    for bad in (['--data', 'a.npy', '--axis', 'up'], ['--data', 'a.npy', '--r_bins', '300'], ['--data', 'a.npy', '--box', '1,2'],
                ['--data', 'a.npy', '--frames', '5:5'], ['--data', 'a.npy', '--r_max', '7'], ['--axis', 'x']):
        with pytest.raises(SystemExit):
            flowstats.get_args(bad)
    own, _ = simulate.get_args(['--seeds', '0:2', '--flow-stats', 'f.json', '--flow-axis', 'auto', '--frames', '40'])
    assert own.flow_stats == 'f.json' and own.flow_axis == 'auto' and own.stats is None and own.pair_stats is None
    own, _ = simulate.get_args(['--frames', '40'])
    assert own.flow_stats is None and own.flow_axis == (1.0, 0.0)
    with pytest.raises(SystemExit):
        simulate.get_args(['--flow-stats', 'f.json', '--flow-axis', 'sideways'])


def test_library_exports_and_rejects_bad_arguments():
    from test_abi import declared_symbols
    from piml_amd import _lib
    names = {'piml_flow_stats', 'piml_flow_stats_workspace_bytes'}
    assert names <= set(declared_symbols()) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    fake = 1 << 20          # never dereferenced: every call below returns before any HIP call
    inf, nan = float('inf'), float('nan')

    def call(S=1, T=2, N=3, t0=0, t1=2, vm=0.1, rb=0.1, RB=4, rmax=0.4, ex=1.0, ey=0.0, lw=0.5, ll=5.0, box=0, x1=1.,
             y0=0., cell=0.5, gx=2, gy=2, nul=fake, mp=fake, wsb=1 << 20):
        return L.piml_flow_stats(nul, fake, fake, None, S, T, N, t0, t1, vm, rb, RB, rmax, ex, ey, lw, ll, box, 0., x1, y0,
                                 1., cell, gx, gy, fake, fake, fake, fake, fake, fake, fake, fake, mp, fake, fake, fake, wsb,
                                 None)
    for bad in (dict(S=-1), dict(T=-1), dict(N=-1), dict(N=65537), dict(t0=-1), dict(t1=3), dict(t0=2, t1=1), dict(vm=0.0),
                dict(vm=nan), dict(rb=0.0), dict(rb=inf), dict(RB=0), dict(RB=257), dict(rmax=0.0), dict(rmax=nan),
                dict(ex=1.01), dict(ex=0.0), dict(ex=nan), dict(ex=0.7, ey=0.7), dict(lw=0.0), dict(ll=-1.0), dict(ll=inf),
                dict(box=1, x1=0.), dict(box=1, y0=2.), dict(box=1, cell=0.), dict(box=1, gx=0), dict(box=1, x1=inf),
                dict(nul=None), dict(box=1, mp=None), dict(wsb=8)):
        assert call(**bad) == 1, bad
    # nothing to do: success, before the buffers are looked at
    for noop in (dict(S=0), dict(N=0), dict(t0=1, t1=1), dict(T=0, t1=0), dict(S=0, nul=None, wsb=0)):
        assert call(**noop) == 0, noop
    assert call(ex=0.6, ey=0.8, S=0) == 0 and call(ex=0.70711, ey=0.70711, N=0) == 0
    assert L.piml_flow_stats_workspace_bytes(2, 5, 3, 4) == 2 * (2 * 5 + 3 * 12) * 8
    assert L.piml_flow_stats_workspace_bytes(2, 5, 0, 0) == 2 * 10 * 8
    assert L.piml_flow_stats_workspace_bytes(2, -1, 0, 0) == -1


def test_new_kernels_use_no_scratch():
    from piml_amd import _lib
    use = _lib.kernel_resource_usage()
    for name in ('flow_stats_kernel', 'flow_stats_copy_kernel'):
        assert name in use, name
        assert use[name]['scratch_bytes'] == 0 and use[name]['vgpr_spill'] == 0, (name, use[name])
