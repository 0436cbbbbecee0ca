"""Is the gfx950 device code of every csrc/*.hip the same as at another commit?  `python tools/isa_identity.py [REV]`
(default HEAD; needs hipcc, no GPU).  Both trees are compiled with build.py's flags plus `--cuda-device-only -S`, the
`__hip_cuid_<hash>` symbol (a hash of the source file) is replaced by a fixed token, and one markdown row per file is
printed: sha256 of the normalised assembly before and after.  ISA_KEEP=<dir> keeps the .s files.  Exit status 1 if any differs."""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from piml_amd import build as B


def asm(tree, name, out):
    src, s = os.path.join(tree, 'piml_amd', 'csrc', name), os.path.join(out, name + '.s')
    if not os.path.exists(src):
        return None
    os.makedirs(out, exist_ok=True)
    subprocess.check_call([B._hipcc()] + B.CFLAGS + B.FILE_FLAGS.get(name, []) + ['--cuda-device-only', '-S', src, '-o', s])
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', open(s).read())
    open(s, 'w').write(text)
    return hashlib.sha256(text.encode()).hexdigest()


rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD'
with tempfile.TemporaryDirectory() as tmp:
    out, old = os.environ.get('ISA_KEEP') or tmp, os.path.join(tmp, 'tree')
    os.makedirs(old)
    tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'piml_amd/csrc', 'include'], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
    names = sorted(os.path.basename(s) for s in B.sources())
    with ThreadPoolExecutor(int(os.environ.get('PIML_BUILD_JOBS', '4'))) as ex:
        rows = list(ex.map(lambda n: (n, asm(old, n, os.path.join(out, 'before')), asm(ROOT, n, os.path.join(out, 'after'))), names))
print(f'| file | sha256 at {rev} | sha256 of this tree | same |\n|---|---|---|---|')
for n, a, b in rows:
    print(f'| {n} | {a} | {b} | {"yes" if a == b else "NO"} |')
sys.exit(any(a != b for _, a, b in rows))
