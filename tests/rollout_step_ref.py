"""One frame of the reference's inference rollout (src/models/simulators.py:595-652) restated in numpy float32, one rounding
per operation, written from the reference's lines (the line numbers stand next to each statement) and not from the kernel
that fuses them (rollout_step_agent, piml_amd/csrc/pairwise.hip).

A case's `data` (tests/rollout_step_shapes.py) is turned into numpy once (`series`), the state of frame t_start is
`initial_state`, and `step` takes the state through one frame given the network's output of that frame.  What the reference
leaves to `get_relative_features` is restated only as far as it touches the state: the NaN -> 0 it writes into the
velocity and acceleration it is handed (src/data/data.py:483-484, the views of :643) and dest_features = destination -
position with NaN -> 0 (:496-497), which the reference puts in front of the row of :651.

Two parameters go beyond the reference: `remove_arrived` (False: an arrived agent keeps walking, :611 is skipped) and
waypoints shared by the slices of a channelled state, (D, N, 2) with a (C, N) index, which the reference's gather of :616
cannot run."""
import types

import numpy as np

F32 = np.float32


def series(data):
    """the fields of `data` a rollout reads, as numpy: the time series, the waypoints, the entry flags"""
    s = types.SimpleNamespace()
    for k in ('position', 'velocity', 'acceleration', 'destination', 'self_features', 'waypoints'):
        s.__dict__[k] = getattr(data, k).detach().cpu().numpy().astype(F32)
    s.dest_idx = data.dest_idx.detach().cpu().numpy().astype(np.int64)
    s.dest_num = data.dest_num.detach().cpu().numpy().astype(np.int64)
    mask_p = data.mask_p.detach().cpu().numpy()
    s.mask_p = mask_p
    s.new_flag = (mask_p - data.mask_p_pred.detach().cpu().numpy()).astype(np.int64)       # :593
    s.T = int(data.num_frames)
    s.dt = F32(data.time_unit)                    # a float32 tensor times a Python float: the float is rounded to float32
    return s


def initial_state(s, t_start):
    """:571-591: the state of frame t_start and the result buffers, rows 0..t_start prefilled from the series"""
    st = types.SimpleNamespace()
    st.t = int(t_start)
    st.p = s.position[..., t_start, :, :].copy()
    st.v = s.velocity[..., t_start, :, :].copy()
    st.a = s.acceleration[..., t_start, :, :].copy()
    st.dest = s.destination[..., t_start, :, :].copy()
    st.dest_idx = s.dest_idx[..., t_start, :].copy()
    sf = s.self_features[..., t_start, :, :]
    st.hist = sf[..., 2:-3].copy()
    st.v0 = sf[..., -1:].copy()
    st.p_res, st.v_res, st.a_res = (np.zeros_like(x) for x in (s.position, s.velocity, s.acceleration))
    st.p_res[..., :t_start + 1, :, :] = s.position[..., :t_start + 1, :, :]
    st.v_res[..., :t_start + 1, :, :] = s.velocity[..., :t_start + 1, :, :]
    st.a_res[..., :t_start + 1, :, :] = s.acceleration[..., :t_start + 1, :, :]
    st.mask = np.zeros(s.mask_p.shape, F32)
    st.mask[..., :t_start + 1, :] = s.mask_p[..., :t_start + 1, :].astype(np.int64)
    return st


def gather_waypoints(waypoints, dest_idx):
    """:614-616 for waypoints (*c, D, N, 2) with an index (*c, N); and (D, N, 2) with an index (C, N)"""
    if waypoints.ndim == dest_idx.ndim + 2:
        idx = np.broadcast_to(dest_idx[..., None, :, None], dest_idx.shape[:-1] + (1, dest_idx.shape[-1], 2))
        return np.take_along_axis(waypoints, idx, axis=-3).squeeze(-3)
    assert waypoints.ndim == 3 and dest_idx.ndim == 2
    return waypoints[dest_idx, np.arange(dest_idx.shape[-1])]


def step(st, s, a_next, remove_arrived=True):
    """One frame on `st` in place (st.t advances).  Returns (self_features[..., 2:] of the next frame, events), events the
    boolean (*c, N) arrays `near` (the index was raised, :609), `gone` (arrived at the last waypoint, :611), `enter`
    (injected, :632) and the float64 distance the switch compared."""
    t = st.t
    p, v, a, dest = st.p, st.v, st.a, st.dest
    st.p_res[..., t, :, :] = p                                                  # :596
    st.v_res[..., t, :, :] = v
    st.a_res[..., t, :, :] = a
    st.mask[..., t, :][~np.isnan(p[..., 0])] = 1                                # :600

    a_next = np.array(a_next, F32)                                              # :602, the network's output
    with np.errstate(invalid='ignore'):
        v_next = (v + (a * s.dt).astype(F32)).astype(F32)                       # :603
        p_next = (p + (v * s.dt).astype(F32)).astype(F32)                       # :604
        d = (p - dest).astype(F32)
        dis = np.sqrt(((d[..., 0] * d[..., 0]).astype(F32) + (d[..., 1] * d[..., 1]).astype(F32)).astype(F32))   # :608
        near = dis < F32(0.5)
        d64 = p.astype(np.float64) - dest.astype(np.float64)
        dist64 = np.hypot(d64[..., 0], d64[..., 1])
    dest_idx = st.dest_idx + near                                               # :609
    gone = dest_idx > s.dest_num - 1
    if remove_arrived:
        p_next[gone] = np.nan                                                   # :611
    dest_idx = dest_idx - gone                                                  # :613
    dest = gather_waypoints(s.waypoints, dest_idx).copy()                       # :614-616
    p, v, a = p_next, v_next, a_next                                            # :619-621
    hist = np.concatenate((st.hist[..., 2:], v), axis=-1)                       # :624-626
    enter = np.zeros(near.shape, bool)
    if t < s.T - 1:                                                             # :629
        enter = s.new_flag[..., t + 1, :] == 1
        if enter.sum() > 0:
            p[enter] = s.position[..., t + 1, :, :][enter]                      # :632-636
            v[enter] = s.velocity[..., t + 1, :, :][enter]
            a[enter] = s.acceleration[..., t + 1, :, :][enter]
            dest[enter] = s.destination[..., t + 1, :, :][enter]
            dest_idx[enter] = s.dest_idx[..., t + 1, :][enter]
            hist[enter] = s.self_features[..., t + 1, :, 2:-3][enter]           # :639
    a[np.isnan(a)] = 0                                                          # data.py:483-484, through the views of :643
    v[np.isnan(v)] = 0
    st.p, st.v, st.a, st.dest, st.dest_idx, st.hist = p, v, a, dest, dest_idx, hist
    st.t = t + 1
    events = types.SimpleNamespace(near=near, gone=gone, enter=enter, dist=dist64)
    return np.concatenate((hist, a, st.v0), axis=-1), events                    # :651


def dest_features(st):
    """:496-497: destination - position with NaN -> 0, the first two columns of the row of :651"""
    with np.errstate(invalid='ignore'):
        f = (st.dest - st.p).astype(F32)
    f[np.isnan(f)] = 0
    return f


def run(s, a_table, t_start=0, remove_arrived=True, frames=None):
    """Every frame from t_start on.  Returns (state after the last frame, per-frame records): a record holds the state after
    the frame (p, v, a, dest, dest_idx, hist), the self_features of the NEXT frame (all columns) and the frame's events."""
    st = initial_state(s, t_start)
    out = []
    for t in range(t_start, s.T if frames is None else t_start + frames):
        tail, ev = step(st, s, a_table[..., t, :, :], remove_arrived)
        out.append(types.SimpleNamespace(selff=np.concatenate((dest_features(st), tail), axis=-1), events=ev,
                                         **{k: getattr(st, k).copy() for k in ('p', 'v', 'a', 'dest', 'dest_idx', 'hist')}))
    return st, out


def differs(got, want):
    """how many entries of two arrays differ: floats bit for bit, a NaN equal to any NaN; -1 on a shape mismatch"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return -1
    if want.dtype.kind != 'f':
        return int((got != want).sum())
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    nan = np.isnan(want)
    return int((np.isnan(got) != nan).sum() + ((got.view(np.uint32) != want.view(np.uint32)) & ~nan).sum())


def state_differences(st, record, final, t, head=False, mask_fill=0):
    """the buffers of a torch rollout state (BaseSimulator._rollout_state) that differ from the restatement after frame t
    (`record` of that frame, `final` the restatement's state after its last frame: a result row is written once): the state,
    self_features[..., 2:] (every column with `head`) and row t of the result buffers -> {name: entries that differ}.
    `mask_fill`: what row t of the mask held before the frame where the restatement's held 0 (the frame writes the ones only)"""
    lo = 0 if head else 2
    pairs = {k: (getattr(st, k), getattr(record, k)) for k in ('p', 'v', 'a', 'dest', 'dest_idx', 'hist')}
    pairs['selff'] = (st.selff[..., lo:], record.selff[..., lo:])
    for k, got, want in (('p_res', st.p_res, final.p_res), ('v_res', st.v_res, final.v_res), ('a_res', st.a_res, final.a_res)):
        pairs[k + '[t]'] = (got[..., t, :, :], want[..., t, :, :])
    pairs['mask[t]'] = (st.mask_new[..., t, :], np.where(final.mask[..., t, :] == 1, F32(1), F32(mask_fill)))
    out = {k: differs(got.detach().cpu().numpy(), want) for k, (got, want) in pairs.items()}
    return {k: n for k, n in out.items() if n != 0}
