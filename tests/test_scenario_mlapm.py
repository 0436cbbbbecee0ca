"""CPU: the MLAPM scenario frame's C ABI (declared, bound, argument checks that return before any HIP call), the simulate
CLI's --law / --params, the law's Python checks, and the gfx950 build of the frame kernel without scratch."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from conftest import REPO


def _header():
    return open(os.path.join(REPO, 'include', 'piml_hip.h')).read()


def test_header_declares_and_lib_binds_the_entry():
    from piml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    assert re.search(r'\bint piml_scenario_step_mlapm\s*\(', text)
    assert 'typedef struct piml_mlapm_law' in text
    assert 'piml_scenario_step_mlapm' in _lib.SIGNATURES
    assert [f for f, _ in _lib.MlapmLaw._fields_] == ['variant', 'tau', 'A', 'B', 'C', 'D', 'theta_deg', 'radius']


def test_abi_checks_without_gpu():
    from piml_amd import _lib, ops_scenario
    L = _lib.lib()
    law = ops_scenario.mlapm_law()
    seeds = (ctypes.c_uint64 * 1)(0)
    s = _lib.Scenario()                                  # all-zero descriptor: capacity 0
    assert L.piml_scenario_step_mlapm(None, None, 1, seeds, ctypes.byref(law), 0, None) == 1
    assert L.piml_scenario_step_mlapm(ctypes.byref(s), None, 1, seeds, ctypes.byref(law), 0, None) == 1
    assert L.piml_scenario_step_mlapm(ctypes.byref(s), None, 1, seeds, None, 0, None) == 1
    assert L.piml_scenario_step_mlapm(ctypes.byref(s), None, 1, None, ctypes.byref(law), 0, None) == 1
    assert L.piml_scenario_step_mlapm(ctypes.byref(s), None, 0, seeds, ctypes.byref(law), 0, None) == 1
    assert L.piml_scenario_step_mlapm(ctypes.byref(s), None, 1, seeds, ctypes.byref(law), -1, None) == 1


@pytest.mark.parametrize('bad', [dict(version='SFM'), dict(tau=0.0), dict(tau=-1.0), dict(tau=float('inf')),
                                 dict(A=float('nan')), dict(B=float('inf')), dict(C=float('nan')), dict(D=float('-inf')),
                                 dict(theta=float('nan')), dict(radius=0.0), dict(radius=-0.3), dict(radius=float('inf'))])
def test_law_rejects(bad):
    from piml_amd import ops_scenario
    with pytest.raises(ValueError):
        ops_scenario.mlapm_law(**bad)


def _calibrate_json(path, **kw):
    from piml_amd import calibrate
    d = {'version': 'UCY', **calibrate.DEFAULT_INIT, 'A': 5.25, **kw}       # the keys calibrate --out writes
    with open(path, 'w') as fh:
        json.dump(d, fh, indent=1)
    return str(path)


def test_cli_parses_law_and_params(tmp_path):
    from piml_amd import simulate
    own, _ = simulate.get_args(['--law', 'mlapm', '--params', _calibrate_json(tmp_path / 'p.json'), '--seeds', '0:4',
                                '--out', 'x_{seed}.npy'])
    assert own.law == 'mlapm' and own.seeds == [0, 1, 2, 3]
    assert own.mlapm['version'] == 'UCY' and own.mlapm['A'] == 5.25 and own.mlapm['theta'] == 56.0
    own, _ = simulate.get_args(['--law', 'mlapm'])                      # main_mlapm.py's constants, version GC
    assert own.mlapm == {'version': 'GC', 'tau': 0.5, 'A': 7.55, 'B': -3.0, 'C': 0.2, 'D': -0.3, 'theta': 56.0}


def test_cli_defaults_to_the_network():
    from piml_amd import simulate
    own, _ = simulate.get_args([])
    assert own.law == 'pinnsf' and own.params is None and not hasattr(own, 'mlapm')


@pytest.mark.parametrize('argv', [['--law', 'mlapm', '--checkpoint', 'x.pt'], ['--params', 'PARAMS'],
                                  ['--law', 'sfm']])
def test_cli_rejects(argv, tmp_path):
    from piml_amd import simulate
    argv = [_calibrate_json(tmp_path / 'p.json') if a == 'PARAMS' else a for a in argv]
    with pytest.raises(SystemExit):
        simulate.get_args(argv)


@pytest.mark.parametrize('content', [{'version': 'SFM'}, {'version': 'GC', 'E': 1.0}, {'version': 'GC', 'A': 'big'},
                                     [1, 2, 3]])
def test_cli_rejects_params_file(content, tmp_path):
    from piml_amd import simulate
    path = tmp_path / 'bad.json'
    path.write_text(json.dumps(content))
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'mlapm', '--params', str(path)])
    with pytest.raises(SystemExit):
        simulate.get_args(['--law', 'mlapm', '--params', str(tmp_path / 'missing.json')])


def test_frame_kernel_builds_for_gfx950_without_scratch(tmp_path):
    from piml_amd import build
    src = os.path.join(REPO, 'piml_amd', 'csrc', 'scenario.hip')
    p = subprocess.run([build._hipcc()] + build.CFLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                          '-o', str(tmp_path / 'scenario.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    report = re.findall(r'Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)', p.stderr)
    names = [n for n, _ in report if n]
    scratch = [int(s) for _, s in report if s]
    assert len(names) == len(scratch) and any('scenario_mlapm_kernel' in n for n in names), names
    assert sum('scenario_frame_kernel' in n for n in names) == 2, names         # one instantiation per scene law
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
