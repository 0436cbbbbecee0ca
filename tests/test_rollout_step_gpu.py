"""The inference-rollout step kernels (piml_rollout_step, piml_rollout_step_ksum: rollout_step_agent, piml_amd/csrc/pairwise.hip)
frame by frame on the cases of tests/rollout_step_shapes.py, against the numpy restatement of the reference's frame
(tests/rollout_step_ref.py, itself bitwise the reference's recorded run: tests/test_rollout_step_ref.py) -- bit for bit, a NaN
equal to any NaN: every operation of the step is one correctly rounded float32 operation, a copy or integer work."""
import types

import numpy as np
import pytest
import torch

from conftest import golden

import rollout_step_ref as R
import rollout_step_shapes as SH
from test_rollout_step_ref import make_simulator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -777.0
INVALID_VALUE = 1                    # hipErrorInvalidValue


def on_device(data):
    out = SH.clone(data)
    for k, v in out.__dict__.items():
        if isinstance(v, torch.Tensor):
            out.__dict__[k] = v.to(DEV)
    return out


def make_state(name):
    """(data on the device, a_table on the device, t_start, rollout state with the result rows above t_start set to SENTINEL)"""
    data, a_table, t_start = SH.case(name)
    data = on_device(data)
    st = make_simulator(None, DEV)._rollout_state(data, t_start)
    for buf in (st.p_res, st.v_res, st.a_res):
        buf[..., t_start + 1:, :, :] = SENTINEL
    st.mask_new[..., t_start + 1:, :] = SENTINEL
    return data, a_table.to(DEV), t_start, st


def read_only(st):
    """copies of what a launch must not write: the series, the waypoints, the entry flags, dest_num, the desired speed and
    the first two columns of self_features"""
    out = {k: v.clone() for k, v in st.series.items()}
    out.update(waypoints=st.waypoints.clone(), new_flag=st.new_flag_u8.clone(), dest_num=st.dest_num.clone(),
               desired_speed=st.desired_speed.clone(), head=st.selff[..., :2].clone())
    return out


def assert_read_only(st, before):
    now = read_only(st)
    for k, v in before.items():
        assert R.differs(now[k].cpu().numpy(), v.cpu().numpy()) == 0, f'{k} was written'


def writable(st):
    return {k: getattr(st, k).clone() for k in ('p', 'v', 'a', 'dest', 'dest_idx', 'hist', 'selff', 'p_res', 'v_res', 'a_res',
                                                 'mask_new', 't')}


def step_frames(name, remove_arrived=True):
    from piml_amd import ops
    data, a_table, t_start, st = make_state(name)
    final, rec = SH.restated(name, remove_arrived)
    before = read_only(st)
    T = data.num_frames
    for t in range(t_start, T):                                  # the counter never reaches T: the kernel indexes by it unguarded
        assert int(st.t) == t < T
        ops.rollout_step(st, data, a_table[..., t, :, :].contiguous(), remove_arrived=remove_arrived)
        st.t.add_(1)
        diff = R.state_differences(st, rec[t - t_start], final, t, mask_fill=SENTINEL if t > t_start else 0)
        assert diff == {}, (name, t, diff)
        for k in ('p_res', 'v_res', 'a_res', 'mask_new'):
            above = getattr(st, k)[..., t + 1:, :] if k == 'mask_new' else getattr(st, k)[..., t + 1:, :, :]
            assert bool((above == SENTINEL).all()), f'{name}: frame {t} wrote {k} above its row'
        assert_read_only(st, before)
    for k, want in (('p_res', final.p_res), ('v_res', final.v_res), ('a_res', final.a_res)):
        assert R.differs(getattr(st, k).cpu().numpy(), want) == 0, k
    return final


@pytest.mark.parametrize('name', SH.ALL)
def test_step_equals_restatement_frame_by_frame(name):
    """After every frame: p, v, a, dest, dest_idx, hist, self_features[..., 2:] and row t of the result buffers equal the
    restatement's; the rows above t, self_features[..., :2], the series and the waypoints were not written."""
    step_frames(name)


def test_step_keeps_arrived_agents_walking_without_remove_arrived():
    final = step_frames('multi_wp', remove_arrived=False)
    data, _, _ = SH.case('multi_wp')
    i = SH.ROLES['one_wp']
    _, rec = SH.restated('multi_wp', False)
    assert any(r.events.gone[i] for r in rec)
    assert not np.isnan(final.p_res[:, i]).any() and all(r.dest_idx[i] == int(data.dest_num[i]) - 1 for r in rec)


class DeviceTableModel:
    """stands where the network does: row k of a_table, k a one-element counter on the device advanced in place, so that a
    captured frame replays with the next row"""

    def __init__(self, a_table, t_start):
        self.axis = a_table.dim() - 3
        self.a_table = a_table
        self.k = torch.full((1,), t_start, device=a_table.device, dtype=torch.long)
        self.calls = 0

    def __call__(self, ped_features, obs_features, self_features):
        out = self.a_table.index_select(self.axis, self.k).squeeze(self.axis)
        self.k.add_(1)
        self.calls += 1
        return (out,)


@pytest.mark.parametrize('name', ('multi_wp', 'hist3', 'slices'))
def test_driver_paths_equal_each_other_and_the_recorded_reference(name):
    """get_multiple_rollouts with a table in the network's place: the eager torch frame, the fused frame and the default
    (fused, captured and replayed where hip_graphs_safe()) give the reference's recorded position, velocity, acceleration
    and mask_p bit for bit."""
    from piml_amd import hip_graphs_safe
    recorded = golden('rollout_step_edges')
    data, a_table, t_start = SH.case(name)
    data, a_table = on_device(data), a_table.to(DEV)
    results, calls = {}, {}
    with torch.no_grad():
        for tag, kw in (('eager', dict(fused=False, use_graph=False)), ('fused', dict(fused=True, use_graph=False)), ('default', {})):
            model = DeviceTableModel(a_table, t_start)
            results[tag] = make_simulator(model, DEV).get_multiple_rollouts(SH.clone(data), t_start=t_start, load_model=False, **kw)
            torch.cuda.synchronize()
            calls[tag] = model.calls
    T = data.num_frames
    assert calls['eager'] == calls['fused'] == T - t_start
    assert calls['default'] == (3 if hip_graphs_safe() else T - t_start)      # two warm-up frames and the captured one
    for tag, res in results.items():
        for k in ('position', 'velocity', 'acceleration', 'mask_p'):
            assert R.differs(getattr(res, k).cpu().numpy(), recorded[f'{name}/{k}']) == 0, (name, tag, k)


KSUM_TAU = 0.5


def ksum_yardstick(sf, pp, po):
    """float64 value of sum pred_ped + sum pred_obs + (v0 d / |d| - v) / tau on the rows `sf` (|d| = 0 reads 0.1), and a float32
    torch evaluation of the same expression"""
    out = []
    for dt in (torch.float64, torch.float32):
        s, p = sf.to(dt), pp.to(dt)
        d, v, v0 = s[:, :2], s[:, 2:4], s[:, 6:7]
        n = torch.norm(d, p=2, dim=-1, keepdim=True)
        n = torch.where(n == 0, n + 0.1, n)
        a = p.sum(-2)
        if po is not None:
            a = a + po.to(dt).sum(-2)
        out.append(a + (v0 * (d / n) - v) / KSUM_TAU)
    return out[0], out[1].double()


@pytest.mark.parametrize('kp', (1, 6))
@pytest.mark.parametrize('ko', (None, 1, 10))
def test_ksum_form(kp, ko):
    """piml_rollout_step_ksum on the `multi_wp` state (F = 7): the state after the launch is the restatement's fed with the
    kernel's own acceleration, bit for bit; that acceleration is the float64 value of sum pred_ped + sum pred_obs +
    (v0 d / |d| - v) / tau on the rows as they stood BEFORE the launch (a thread reads its row before it rewrites it), within
    4 x the largest error of a float32 torch evaluation of the same expression against the same float64 values, relative to the
    largest entry, 1e-6 at the least (the kernel sums its up to 16 terms in another order).  Rows that enter at frame 1 take
    the series' acceleration, rows whose value is NaN (the absent agent's NaN history) carry 0 (data.py:483): they are
    compared with that.  One row has self_features[:2] = (0, 0) exactly, one v0 = 0.
    Measured on an MI355X (kernel error / float32 yardstick, relative to the largest entry; 4 x the yardstick is below the
    floor everywhere, so the bound is 1e-6 in all six):
      kp 1, no obstacles 5.8e-8 / 5.8e-8    kp 1, ko 1  7.0e-8 / 7.0e-8    kp 1, ko 10  8.0e-8 / 7.8e-8
      kp 6, no obstacles 5.9e-8 / 8.3e-8    kp 6, ko 1  5.1e-8 / 5.1e-8    kp 6, ko 10  8.2e-8 / 1.1e-7"""
    from piml_amd import ops
    data, _, t_start, st = make_state('multi_wp')
    N = st.p.shape[0]
    zero_d, zero_v0 = 10, 11
    st.selff[zero_d, :2] = 0
    st.selff[zero_v0, 6] = 0
    g = torch.Generator().manual_seed(400 + 16 * kp + (ko or 0))
    pp = torch.randn(N, kp, 2, generator=g).to(DEV)
    po = None if ko is None else torch.randn(N, ko, 2, generator=g).to(DEV)
    rows = st.selff.clone()
    before = read_only(st)
    ops.rollout_step(st, data, None, ksum=(pp, po, KSUM_TAU))
    st.t.add_(1)
    torch.cuda.synchronize()
    assert_read_only(st, before)

    s = R.series(SH.case('multi_wp')[0])
    ref = R.initial_state(s, t_start)
    a_kernel = st.a.cpu().numpy()
    tail, ev = R.step(ref, s, a_kernel)
    rec = types.SimpleNamespace(selff=np.concatenate((R.dest_features(ref), tail), -1),
                                **{k: getattr(ref, k) for k in ('p', 'v', 'a', 'dest', 'dest_idx', 'hist')})
    assert R.state_differences(st, rec, ref, t_start) == {}

    want, f32 = ksum_yardstick(rows.cpu(), pp.cpu(), None if po is None else po.cpu())
    plain = torch.from_numpy(~ev.enter) & ~want.isnan().any(-1)
    assert int(plain.sum()) >= N - 6 and bool(plain[zero_d]) and bool(plain[zero_v0])
    scale = float(want[plain].abs().max())
    yard = float((f32 - want)[plain].abs().max()) / scale
    err = float((torch.from_numpy(a_kernel).double() - want)[plain].abs().max()) / scale
    bound = max(4 * yard, 1e-6)
    print(f'ksum kp={kp} ko={ko}: kernel error {err:.2e}, float32 yardstick {yard:.2e}, bound {bound:.2e}')
    assert err <= bound, (err, yard, bound)
    gone_nan = torch.from_numpy(~ev.enter) & want.isnan().any(-1)
    assert bool(gone_nan[SH.ROLES['never']]) and bool((st.a.cpu()[gone_nan] == 0).all())
    enter = torch.from_numpy(ev.enter)
    assert R.differs(a_kernel[ev.enter], s.acceleration[t_start + 1][ev.enter]) == 0 and int(enter.sum()) >= 1


def raw_args(st, data, a_next, **over):
    """the argument list of piml_rollout_step as ops.rollout_step builds it, with entries replaced by name"""
    from piml_amd.ops import _ptr, _stream
    wp = data.waypoints
    C = st.p.numel() // max(st.p.shape[-2] * 2, 1)
    named = dict(
        p=_ptr(st.p), v=_ptr(st.v), a=_ptr(st.a), dest=_ptr(st.dest), dest_idx=_ptr(st.dest_idx), hist=_ptr(st.hist),
        hist_width=st.hist.shape[-1], a_next=_ptr(a_next), waypoints=_ptr(st.waypoints), D=wp.shape[-3],
        per_slice=int(wp.dim() > 3), dest_num=_ptr(st.dest_num), pos_s=_ptr(st.series['position']),
        vel_s=_ptr(st.series['velocity']), acc_s=_ptr(st.series['acceleration']), dest_s=_ptr(st.series['destination']),
        idx_s=_ptr(st.series['dest_idx']), selff_s=_ptr(st.series['self_features']), F=st.selff.shape[-1],
        new_flag=_ptr(st.new_flag_u8), p_res=_ptr(st.p_res), v_res=_ptr(st.v_res), a_res=_ptr(st.a_res),
        mask=_ptr(st.mask_new), selff=_ptr(st.selff), v0=_ptr(st.desired_speed), t=_ptr(st.t), C=C, T=st.T, N=st.p.shape[-2],
        dt=float(data.time_unit), remove_arrived=1, stream=_stream())
    assert set(over) <= set(named), over
    named.update(over)
    return list(named.values())


def assert_refused(code, st, before_w, before_r):
    from piml_amd import _lib
    assert code == INVALID_VALUE
    with pytest.raises(_lib.PimlHipError):
        _lib.check(code, 'piml_rollout_step')
    torch.cuda.synchronize()
    now = writable(st)
    for k, v in before_w.items():
        assert R.differs(now[k].cpu().numpy(), v.cpu().numpy()) == 0, f'{k} was written'
    assert_read_only(st, before_r)


@pytest.mark.parametrize('over', (dict(hist_width=1), dict(F=8), dict(D=0), dict(T=0)), ids=lambda o: '-'.join(f'{k}{v}' for k, v in o.items()))
def test_step_refuses_bad_arguments(over):
    """the library's invalid-value error, nothing written"""
    from piml_amd import _lib
    data, a_table, t_start, st = make_state('multi_wp')
    bw, br = writable(st), read_only(st)
    with torch.cuda.device(DEV):
        code = _lib.lib().piml_rollout_step(*raw_args(st, data, a_table[..., t_start, :, :].contiguous(), **over))
    assert_refused(code, st, bw, br)


@pytest.mark.parametrize('case', ('F11', 'kp0', 'tau0', 'null_pred_ped', 'hist_width1', 'D0', 'T0'))
def test_ksum_step_refuses_bad_arguments(case):
    from piml_amd import _lib
    from piml_amd.ops import _ptr
    data, _, _, st = make_state('hist3' if case == 'F11' else 'multi_wp')       # F = 11 = hist_width + 5 passes the shared check
    assert st.selff.shape[-1] == (11 if case == 'F11' else 7)
    N = st.p.shape[0]
    pp, po = torch.randn(N, 6, 2, device=DEV), torch.randn(N, 10, 2, device=DEV)
    head = dict(pred_ped=_ptr(pp), kp=6, pred_obs=_ptr(po), ko=10, tau=KSUM_TAU)
    head.update(dict(kp0=dict(kp=0), tau0=dict(tau=0.0), null_pred_ped=dict(pred_ped=None)).get(case, {}))
    over = dict(hist_width1=dict(hist_width=1), D0=dict(D=0), T0=dict(T=0)).get(case, {})
    bw, br = writable(st), read_only(st)
    with torch.cuda.device(DEV):
        code = _lib.lib().piml_rollout_step_ksum(*head.values(), *raw_args(st, data, None, **over))
    assert_refused(code, st, bw, br)


@pytest.mark.parametrize('over', (dict(C=0), dict(N=0)), ids=('C0', 'N0'))
@pytest.mark.parametrize('ksum', (False, True))
def test_empty_step_succeeds_and_writes_nothing(over, ksum):
    from piml_amd import _lib
    from piml_amd.ops import _ptr
    data, a_table, t_start, st = make_state('multi_wp')
    N = st.p.shape[0]
    pp = torch.randn(N, 6, 2, device=DEV)
    bw, br = writable(st), read_only(st)
    with torch.cuda.device(DEV):
        if ksum:
            code = _lib.lib().piml_rollout_step_ksum(_ptr(pp), 6, None, 1, KSUM_TAU, *raw_args(st, data, None, **over))
        else:
            code = _lib.lib().piml_rollout_step(*raw_args(st, data, a_table[..., t_start, :, :].contiguous(), **over))
    assert code == 0
    torch.cuda.synchronize()
    now = writable(st)
    for k, v in bw.items():
        assert R.differs(now[k].cpu().numpy(), v.cpu().numpy()) == 0, f'{k} was written'
    assert_read_only(st, br)
