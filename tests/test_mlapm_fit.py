"""CPU-only: packing a clip for the MLAPM calibration (piml_amd.calibrate.pack_clip), the C ABI of the fit kernel
(exported, arguments refused before any launch) and the command line."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO


def toy_raw():
    """4 frames, 3 agents: agent 0 everywhere, agent 1 absent in frame 2, agent 2 from frame 1 on with its last frame
    without a velocity (mask_v = 0, the loader's placeholder)."""
    from piml_amd.data.data import RawData
    nan = float('nan')
    T, N = 4, 3
    p = torch.arange(T * N * 2, dtype=torch.float32).reshape(T, N, 2) / 10
    v = torch.ones(T, N, 2) + torch.arange(T, dtype=torch.float32).reshape(T, 1, 1)
    d = torch.full((T, N, 2), 50.0)
    p[2, 1] = nan
    d[2, 1] = nan
    p[0, 2] = nan
    v[0, 2] = 0.0
    raw = RawData(position=p, velocity=v, destination=d, meta_data={'time_unit': 0.08})
    raw.mask_v = torch.ones(T, N)
    raw.mask_v[0, 2] = 0
    raw.mask_v[3, 2] = 0
    raw.mask_v[2, 1] = 0
    return raw


def test_pack_clip_layout_and_default_targets():
    from piml_amd.calibrate import pack_clip
    raw = toy_raw()
    pk = pack_clip(raw, desired_speed=torch.tensor([1.0, 2.0, 3.0]), device='cpu')
    # present: t0 {0, 1}, t1 {0, 1, 2}, t2 {0, 2}, t3 {0, 1}
    assert pk.offsets.tolist() == [0, 2, 5, 7, 9]
    assert pk.frame_of.tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3]
    assert pk.agent.tolist() == [0, 1, 0, 1, 2, 0, 2, 0, 1]
    assert pk.state.shape == (9, 4) and pk.state.dtype == torch.float32
    assert torch.equal(pk.state[2, :2], raw.position[1, 0]) and torch.equal(pk.state[2, 2:], raw.velocity[1, 0])
    assert pk.desired_speed.tolist() == [1.0, 2.0, 1.0, 2.0, 3.0, 1.0, 3.0, 1.0, 2.0]
    assert pk.time_unit == pytest.approx(0.08)
    # default target = v of frame t + 1 where the agent is present then
    tg = pk.target
    assert torch.equal(tg[0], raw.velocity[1, 0]) and torch.equal(tg[4], raw.velocity[2, 2])
    finite = torch.isfinite(tg).all(-1).tolist()
    # (t0,0) t1 present; (t0,1) t1 present; (t1,0); (t1,1) absent in t2; (t1,2) t2 present; (t2,0); (t2,2) last frame t3
    # without velocity; (t3, *) no next frame
    assert finite == [True, True, True, False, True, True, False, False, False]
    assert pk.num_focal == 5
    assert sorted(pk.small_focal.tolist()) == [0, 1, 2, 4, 5] and pk.big_focal.numel() == 0


def test_pack_clip_frames_targets_and_desired_speed():
    from piml_amd.calibrate import pack_clip
    from piml_amd.data.data import desired_speed_per_agent
    raw = toy_raw()
    pk = pack_clip(raw, frames='1:3', device='cpu')
    assert pk.frames == [1, 2] and pk.offsets.tolist() == [0, 3, 5] and pk.frame_of.tolist() == [0, 0, 0, 1, 1]
    v = torch.where(torch.isfinite(raw.position).all(-1, keepdim=True) & (raw.mask_v != 0).unsqueeze(-1), raw.velocity,
                    torch.zeros_like(raw.velocity))
    ds = desired_speed_per_agent(v, 25)
    assert torch.equal(pk.desired_speed, ds[pk.agent])
    # a caller's target replaces v_{t+1}; NaN entries drop out of the loss
    tgt = torch.randn(4, 3, 2)
    tgt[1, 2] = float('nan')
    pk = pack_clip(raw, frames=[1], target=tgt, device='cpu')
    assert torch.equal(pk.target[:2], tgt[1, :2]) and pk.num_focal == 2 and pk.small_focal.tolist() == [0, 1]
    # frames of more than 64 agents go to the wave-per-agent list
    from piml_amd.data.data import RawData
    big = RawData(position=torch.randn(3, 70, 2), velocity=torch.randn(3, 70, 2), destination=torch.randn(3, 70, 2),
                  meta_data={'time_unit': 0.1})
    pk = pack_clip(big, device='cpu')
    assert pk.offsets.tolist() == [0, 70, 140, 210] and pk.small_focal.numel() == 0 and pk.big_focal.tolist() == list(range(140))


def test_desired_speed_rule_of_make_dataset():
    """The shared helper keeps TimeIndexedPedData.make_dataset's rule: the mean |v| over skip_frames frames after the start."""
    from piml_amd.data.data import desired_speed_per_agent
    v = torch.zeros(6, 2, 2)
    v[2:, 0, 0] = torch.tensor([1.0, 3.0, 5.0, 7.0])
    assert desired_speed_per_agent(v, 2).tolist() == [2.0, 0.0]
    assert desired_speed_per_agent(v, 25).tolist() == [4.0, 0.0]


def test_fit_abi_exported_and_arguments_refused():
    from piml_amd import _lib
    L = _lib.lib()
    assert 'piml_mlapm_fit_loss_grad' in _lib.SIGNATURES and 'piml_mlapm_fit_workspace_doubles' in _lib.SIGNATURES
    assert L.piml_mlapm_fit_workspace_doubles(0, 0) == 0
    assert L.piml_mlapm_fit_workspace_doubles(1, 0) == 8 and L.piml_mlapm_fit_workspace_doubles(257, 5) == 8 * (2 + 2)
    assert L.piml_mlapm_fit_workspace_doubles(-1, 0) == -1
    fake = 4096          # never dereferenced: every call below is refused before a launch

    def call(E=4, F=1, n_small=2, n_big=0, variant=1, dt=0.08, radius=0.3, ws=fake, ws_n=8, params=fake, bufs=fake):
        return L.piml_mlapm_fit_loss_grad(bufs, bufs, bufs, bufs, bufs, bufs, E, F, bufs if n_small else None, n_small,
                                          bufs if n_big else None, n_big, params, variant, dt, radius, ws, ws_n, fake, fake, None)
    bad = 1              # hipErrorInvalidValue
    assert call(E=-1) == bad and call(F=-1) == bad and call(n_small=-1) == bad and call(n_big=-1) == bad
    assert call(n_small=3, n_big=2) == bad                        # more focal entries than entries
    assert call(variant=3) == bad and call(variant=-1) == bad
    assert call(dt=float('nan')) == bad and call(radius=float('inf')) == bad
    assert call(params=None) == bad and call(bufs=None) == bad
    assert call(ws=None) == bad and call(ws_n=7) == bad           # workspace missing / too small


def test_ops_refuses_cpu_pack():
    from piml_amd import ops
    from piml_amd._lib import PimlHipError
    from piml_amd.calibrate import pack_clip
    pk = pack_clip(toy_raw(), device='cpu')
    with pytest.raises((PimlHipError, TypeError)):
        ops.mlapm_fit_loss_grad(pk, torch.zeros(6), 'GC', 0.08, 0.3)
    with pytest.raises(NotImplementedError):
        ops.mlapm_fit_loss_grad(pk, torch.zeros(6), 'SFM', 0.08, 0.3)


def test_cli_help_and_parsing():
    from piml_amd import calibrate as C
    a = C.get_args(['--data', 'clip.npy', '--version', 'UCY', '--init', 'A=7.55,B=-3,theta=40', '--fit', 'A,B,theta',
                    '--frames', '10:200', '--valid_frames', '200:300', '--steps', '40', '--out', 'p.json'])
    assert a.version == 'UCY' and a.init == {'A': 7.55, 'B': -3.0, 'theta': 40.0} and a.fit == ('A', 'B', 'theta')
    assert a.frames == '10:200' and a.valid_frames == '200:300' and a.steps == 40 and a.out == 'p.json'
    a = C.get_args(['--data', 'x.npy'])
    assert a.version == 'GC' and a.fit == C.PARAM_NAMES and a.init == {}
    for bad in (['--init', 'E=1'], ['--init', 'A'], ['--fit', 'A,Z'], ['--version', 'SFM']):
        with pytest.raises(SystemExit):
            C.get_args(['--data', 'x.npy'] + bad)
    assert C._frame_list('2:5', 10) == [2, 3, 4] and C._frame_list(None, 3) == [0, 1, 2]
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, '-m', 'piml_amd.calibrate', '--help'], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and '--valid_frames' in p.stdout and '--fit' in p.stdout
