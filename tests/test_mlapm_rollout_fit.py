"""CPU-only: packing rollout windows for the MLAPM rollout calibration (piml_amd.calibrate.pack_windows), pack_clip of
several clips, the C ABI of the rollout-fit kernel (exported, arguments refused before any launch) and the command line."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO

P_, I_, C_ = 1, 2, 4          # flag bits: present, injected, carried


def toy_raw(time_unit=0.08, shift=0.0):
    """4 frames, 3 agents: agent 0 everywhere, agent 1 absent in frame 2, agent 2 from frame 1 on with its last frame
    without a velocity (mask_v = 0, the loader's placeholder).  Present: t0 {0, 1}, t1 {0, 1, 2}, t2 {0, 2}, t3 {0, 1}."""
    from piml_amd.data.data import RawData
    nan = float('nan')
    T, N = 4, 3
    p = torch.arange(T * N * 2, dtype=torch.float32).reshape(T, N, 2) / 10 + shift
    v = torch.ones(T, N, 2) + torch.arange(T, dtype=torch.float32).reshape(T, 1, 1)
    d = torch.full((T, N, 2), 50.0)
    p[2, 1] = nan
    d[2, 1] = nan
    p[0, 2] = nan
    v[0, 2] = 0.0
    raw = RawData(position=p, velocity=v, destination=d, meta_data={'time_unit': time_unit})
    raw.mask_v = torch.ones(T, N)
    raw.mask_v[0, 2] = 0
    raw.mask_v[3, 2] = 0
    raw.mask_v[2, 1] = 0
    return raw


def test_pack_windows_layout_by_hand():
    from piml_amd.calibrate import pack_windows
    raw = toy_raw()
    pk = pack_windows(raw, 2, desired_speed=torch.tensor([1.0, 2.0, 3.0]), device='cpu')
    # windows t0 = 0 (frames 0..2) and t0 = 1 (frames 1..3); both hold all three agents
    assert pk.start == [0, 1] and pk.num_windows == 2 and pk.slot_count == [3, 3]
    assert pk.slot_offsets.tolist() == [0, 3, 6] and pk.agent.tolist() == [0, 1, 2, 0, 1, 2]
    assert pk.desired_speed.tolist() == [1.0, 2.0, 3.0, 1.0, 2.0, 3.0]
    # entry (w, k, s) = 3 * slot_offsets[w] + 3 k + s
    w0 = [P_ | I_, P_ | I_, 0,                   # k0: agent 2 absent
          P_ | C_, P_ | C_, P_ | I_,             # k1: agent 2 enters
          P_ | C_, 0, P_ | C_]                   # k2: agent 1 absent
    w1 = [P_ | I_, P_ | I_, P_ | I_,
          P_ | C_, 0, P_ | C_,
          P_ | C_, P_ | I_, 0]                   # k2: agent 1 re-enters (injected), agent 2 has no velocity
    assert pk.flags.tolist() == w0 + w1
    assert pk.num_terms == 7 and pk.terms_per_step == [4, 3]
    # recorded (p, v) of frame t0 + k, zeros where absent
    assert torch.equal(pk.rec[3 + 2], torch.cat((raw.position[1, 2], raw.velocity[1, 2])))
    assert torch.equal(pk.rec[9 + 6 + 1], torch.cat((raw.position[3, 1], raw.velocity[3, 1])))
    assert pk.rec[2].tolist() == [0.0] * 4 and pk.destination[2].tolist() == [0.0, 0.0]
    assert torch.isfinite(pk.rec).all() and torch.isfinite(pk.destination).all()
    assert pk.small_windows.tolist() == [0, 1] and pk.big_windows.numel() == 0 and pk.big_slots == 0
    assert pk.time_unit == pytest.approx(0.08) and pk.horizon == 2


def test_pack_windows_range_end_stride_and_frames():
    from piml_amd.calibrate import pack_windows
    raw = toy_raw()
    assert pack_windows(raw, 2, frames='0:3', device='cpu').start == [0]      # t0 + H must lie in the range
    assert pack_windows(raw, 3, device='cpu').start == [0]
    assert pack_windows(raw, 4, device='cpu').num_windows == 0
    assert pack_windows(raw, 1, device='cpu').start == [0, 1, 2]
    assert pack_windows(raw, 1, stride=2, device='cpu').start == [0, 2]
    assert pack_windows(raw, 1, frames=[1, 2, 3], device='cpu').start == [1, 2]
    pk = pack_windows(raw, 1, frames='2:4', device='cpu')
    # frames 2..3: slots {0, 1, 2}; k0 agent 1 absent; k1 agent 1 enters, agent 2 leaves
    assert pk.start == [2] and pk.flags.tolist() == [P_ | I_, 0, P_ | I_, P_ | C_, P_ | I_, 0] and pk.num_terms == 1
    with pytest.raises(ValueError):
        pack_windows(raw, 1, frames=[0, 2, 3], device='cpu')                  # not consecutive
    with pytest.raises(ValueError):
        pack_windows(raw, 0, device='cpu')
    with pytest.raises(ValueError):
        pack_windows(raw, 1, stride=0, device='cpu')


def test_pack_windows_default_speed_and_big_windows():
    from piml_amd.calibrate import pack_windows
    from piml_amd.data.data import RawData, desired_speed_per_agent
    raw = toy_raw()
    pk = pack_windows(raw, 1, device='cpu')
    v = torch.where(torch.isfinite(raw.position).all(-1, keepdim=True) & (raw.mask_v != 0).unsqueeze(-1), raw.velocity,
                    torch.zeros_like(raw.velocity))
    assert torch.equal(pk.desired_speed, desired_speed_per_agent(v, 25)[pk.agent])
    # windows of more than 64 slots go to the wave-per-slot list, with the prefix sum of their slot counts
    g = torch.Generator().manual_seed(0)
    big = RawData(position=torch.randn(4, 70, 2, generator=g), velocity=torch.randn(4, 70, 2, generator=g),
                  destination=torch.randn(4, 70, 2, generator=g), meta_data={'time_unit': 0.1})
    big.position[:2, 69] = float('nan')                   # agent 69 only from frame 2 on
    pk = pack_windows(big, 1, device='cpu')
    assert pk.slot_count == [69, 70, 70] and pk.small_windows.numel() == 0
    assert pk.big_windows.tolist() == [0, 1, 2] and pk.big_base.tolist() == [0, 69, 139] and pk.big_slots == 209
    # beyond the small form's horizon every window is big
    pk = pack_windows(toy_raw(), 1, device='cpu')
    assert pk.small_windows.numel() == 3
    from piml_amd.calibrate import ROLL_SMALL_MAX_H
    long = RawData(position=torch.randn(ROLL_SMALL_MAX_H + 3, 3, 2, generator=g),
                   velocity=torch.randn(ROLL_SMALL_MAX_H + 3, 3, 2, generator=g),
                   destination=torch.randn(ROLL_SMALL_MAX_H + 3, 3, 2, generator=g), meta_data={'time_unit': 0.1})
    pk = pack_windows(long, ROLL_SMALL_MAX_H + 1, device='cpu')
    assert pk.num_windows == 2 and pk.small_windows.numel() == 0 and pk.big_windows.tolist() == [0, 1]


def test_pack_windows_of_two_clips_is_the_concatenation():
    from piml_amd.calibrate import pack_windows
    a, b = toy_raw(), toy_raw(shift=1.0)
    b.position = b.position[:3]
    b.velocity = b.velocity[:3]
    b.destination = b.destination[:3]
    b.mask_v = b.mask_v[:3]
    pa, pb = pack_windows(a, 1, device='cpu'), pack_windows(b, 1, device='cpu')
    pc = pack_windows([a, b], 1, device='cpu')
    assert pc.num_windows == pa.num_windows + pb.num_windows == 5 and pc.clip == [0, 0, 0, 1, 1]
    assert pc.start == pa.start + pb.start                                  # windows never cross clips
    for name in ('rec', 'destination', 'flags', 'desired_speed', 'agent'):
        assert torch.equal(getattr(pc, name), torch.cat((getattr(pa, name), getattr(pb, name)))), name
    assert pc.slot_offsets.tolist() == pa.slot_offsets.tolist() + [x + pa.num_slots for x in pb.slot_offsets.tolist()[1:]]
    assert pc.small_windows.tolist() == pa.small_windows.tolist() + [x + pa.num_windows for x in pb.small_windows.tolist()]
    assert pc.num_terms == pa.num_terms + pb.num_terms
    assert pc.terms_per_step == [x + y for x, y in zip(pa.terms_per_step, pb.terms_per_step)]
    with pytest.raises(ValueError):
        pack_windows([a, toy_raw(time_unit=0.1)], 1, device='cpu')         # time units disagree


def test_pack_clip_of_a_list_is_the_concatenation():
    from piml_amd.calibrate import pack_clip
    a, b = toy_raw(), toy_raw(shift=2.0)
    pa, pb = pack_clip(a, device='cpu'), pack_clip(b, device='cpu')
    assert not hasattr(pa, 'clip')                                          # a single clip: today's pack
    assert pa.offsets.tolist() == [0, 2, 5, 7, 9] and pa.num_focal == 5
    pc = pack_clip([a, b], device='cpu')
    for name in ('state', 'destination', 'desired_speed', 'frame', 'agent'):
        assert torch.equal(getattr(pc, name), torch.cat((getattr(pa, name), getattr(pb, name)))), name
    torch.testing.assert_close(pc.target, torch.cat((pa.target, pb.target)), rtol=0, atol=0, equal_nan=True)
    assert pc.offsets.tolist() == pa.offsets.tolist() + [x + pa.num_entries for x in pb.offsets.tolist()[1:]]
    assert pc.frame_of.tolist() == pa.frame_of.tolist() + [x + len(pa.frames) for x in pb.frame_of.tolist()]
    assert pc.small_focal.tolist() == pa.small_focal.tolist() + [x + pa.num_entries for x in pb.small_focal.tolist()]
    assert pc.num_focal == pa.num_focal + pb.num_focal and pc.frames == pa.frames + pb.frames
    assert pc.clip.tolist() == [0] * pa.num_entries + [1] * pb.num_entries
    with pytest.raises(ValueError):
        pack_clip([a, toy_raw(time_unit=0.1)], device='cpu')
    pd = pack_clip([a, b], desired_speed=[1.0, 2.0], device='cpu')
    assert pd.desired_speed.tolist() == [1.0] * pa.num_entries + [2.0] * pb.num_entries


def test_rollout_abi_exported_and_arguments_refused():
    from piml_amd import _lib
    L = _lib.lib()
    assert 'piml_mlapm_rollout_fit_loss_grad' in _lib.SIGNATURES
    assert 'piml_mlapm_rollout_fit_workspace_doubles' in _lib.SIGNATURES
    ws = L.piml_mlapm_rollout_fit_workspace_doubles
    assert ws(0, 1, 0) == 0
    assert ws(3, 2, 0) == 3 * 12 and ws(1, 1, 0) == 10 and ws(1, 2, 0) == 12
    assert ws(3, 1, 5) == 3 * 10 + 5 * 5 * 2 and ws(1, 8, 1) == 24 + 24
    assert ws(-1, 1, 0) == -1 and ws(1, 0, 0) == -1 and ws(1, 1, -1) == -1
    fake = 4096          # never dereferenced: every call below is refused before a launch

    def call(W=2, S=4, H=2, n_small=1, n_big=1, big_slots=2, variant=1, dt=0.08, radius=0.3, decay=1.0, ws=fake,
             ws_n=1 << 20, params=fake, bufs=fake, offs=fake):
        return L.piml_mlapm_rollout_fit_loss_grad(bufs, bufs, bufs, bufs, offs, W, S, H, bufs if n_small else None, n_small,
                                                  bufs if n_big else None, bufs if n_big else None, n_big, big_slots,
                                                  params, variant, dt, radius, decay, ws, ws_n, fake, fake, None, None)
    bad = 1              # hipErrorInvalidValue
    assert call(W=-1) == bad and call(S=-1) == bad and call(n_small=-1) == bad and call(n_big=-1) == bad
    assert call(H=0) == bad and call(H=-3) == bad and call(big_slots=-1) == bad
    assert call(n_small=2, n_big=1) == bad                          # more windows listed than packed
    assert call(H=49) == bad                                        # small windows hold (H + 3) KiB of LDS, H <= 48
    assert call(variant=3) == bad and call(variant=-1) == bad
    assert call(dt=float('nan')) == bad and call(dt=0.0) == bad and call(dt=-0.1) == bad
    assert call(radius=float('inf')) == bad and call(radius=-1.0) == bad
    assert call(decay=float('nan')) == bad and call(decay=-0.5) == bad
    assert call(params=None) == bad and call(bufs=None) == bad and call(offs=None) == bad
    assert call(ws=None) == bad and call(ws_n=ws(2, 2, 2) - 1) == bad   # workspace missing / too small


def test_ops_refuses_cpu_pack_and_bad_outputs():
    from piml_amd import ops
    from piml_amd._lib import PimlHipError
    from piml_amd.calibrate import pack_windows
    pk = pack_windows(toy_raw(), 2, device='cpu')
    with pytest.raises((PimlHipError, TypeError)):
        ops.mlapm_rollout_fit_loss_grad(pk, torch.zeros(6), 'GC', 0.08, 0.3)
    with pytest.raises(NotImplementedError):
        ops.mlapm_rollout_fit_loss_grad(pk, torch.zeros(6), 'SFM', 0.08, 0.3)


def test_calibrate_refuses_a_cpu_pack_and_a_mismatched_horizon():
    from piml_amd.calibrate import calibrate_mlapm, pack_windows
    pk = pack_windows(toy_raw(), 2, device='cpu')
    with pytest.raises(ValueError):
        calibrate_mlapm(pk, horizon=3)
    with pytest.raises(ValueError):
        calibrate_mlapm(pk, horizon=2)                               # packed on the CPU


def test_cli_parses_rollout_flags_and_several_clips():
    from piml_amd import calibrate as C
    a = C.get_args(['--data', 'a.npy', 'b.npy', 'c.npy', '--horizon', '16', '--stride', '4', '--time_decay', '0.9',
                    '--frames', '0:500', '--valid_frames', '500:700'])
    assert a.data == ['a.npy', 'b.npy', 'c.npy'] and a.horizon == 16 and a.stride == 4 and a.time_decay == 0.9
    a = C.get_args(['--data', 'x.npy'])
    assert a.data == ['x.npy'] and a.horizon is None and a.stride == 1 and a.time_decay == 1.0
    for bad in (['--horizon', 'x'], ['--stride', '1.5']):
        with pytest.raises(SystemExit):
            C.get_args(['--data', 'x.npy'] + bad)
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.calibrate', '--help'], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and '--horizon' in p.stdout and '--time_decay' in p.stdout and '--stride' in p.stdout
