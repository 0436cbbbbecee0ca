"""Driver of tools/probe_store_through.hip: builds the probe (if tools/probe_store_through is missing), runs it under a `timeout`
for the pairs' HIP-event times and prints the table of profiles/r12_store_through.md.  (The probe is not run under a kernel
trace: profiles/r12_store_through.md, "What was not measured".)

    python tools/probe_store_through.py [output directory, default build/probe_store_through]"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tools', 'probe_store_through')
SRC = EXE + '.hip'
MODES = ('plain 16 B', 'write-through 16 B', 'plain 4 B', 'write-through 4 B')


def build():
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '--offload-arch=gfx950',
                           '-I', os.path.join(ROOT, 'piml_amd', 'csrc'), '-o', EXE, SRC])


def main():
    out = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'build', 'probe_store_through'))
    os.makedirs(out, exist_ok=True)
    build()
    if '--build-only' in sys.argv:
        return 0
    log = subprocess.run(['timeout', '-k', '10', '120', EXE], capture_output=True, text=True)
    open(os.path.join(out, 'events.log'), 'w').write(log.stdout + log.stderr)
    if log.returncode != 0:
        print(f'the probe ended with status {log.returncode}; see {out}/events.log')
        return log.returncode
    pair = {}
    for m in re.finditer(r'PAIR mode=(\d) MB=(\d+) shift=(\d) pair_us=([\d.]+)', log.stdout):
        pair[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = float(m.group(4))
    lines = ['| MiB | stores | pair µs, reader on the storing XCD | pair µs, reader on another XCD |', '|---|---|---|---|']
    for mb in (4, 13, 18):
        for mode, name in enumerate(MODES):
            f = lambda d, k: f'{d[k]:.2f}' if k in d else '-'
            lines.append(f'| {mb} | {name} | {f(pair, (mode, mb, 0))} | {f(pair, (mode, mb, 3))} |')
    table = '\n'.join(lines)
    open(os.path.join(out, 'table.md'), 'w').write(table + '\n')
    print(table)
    return 0


if __name__ == '__main__':
    sys.exit(main())
