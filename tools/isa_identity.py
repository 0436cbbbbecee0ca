"""Is the gfx950 device code of every csrc/*.hip the same as at another commit?  `python tools/isa_identity.py [REV]`
(default HEAD; needs hipcc, no GPU).  Both trees are compiled with build.py's flags plus `--cuda-device-only -S`, the
`__hip_cuid_<hash>` symbol (a hash of the source file) is replaced by a fixed token, and one markdown row per file is
printed: sha256 of the normalised assembly before and after.  A file whose hash differs (kernels came or went) or that one
tree lacks is then compared kernel by kernel: the assembly is cut at the function symbols (body up to .Lfunc_end, plus the
.amdhsa_kernel descriptor), the function's ordinal in local labels (.LBB<n>_, .Lfunc_end<n>, ...) is dropped, and one row per
function name says same / DIFFERENT / only before / only after.  ISA_KEEP=<dir> keeps the .s files.  Exit status 1 if a function
present in both trees differs or one is new; functions that are gone are listed for the reader to judge."""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from piml_amd import build as B
from piml_amd._lib import _demangle_lite


def asm(tree, name, out):
    src, s = os.path.join(tree, 'piml_amd', 'csrc', name), os.path.join(out, name + '.s')
    if not os.path.exists(src):
        return None
    os.makedirs(out, exist_ok=True)
    subprocess.check_call([B._hipcc()] + B.CFLAGS + B.FILE_FLAGS.get(name, []) + ['--cuda-device-only', '-S', src, '-o', s])
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', open(s).read())
    open(s, 'w').write(text)
    return text


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest() if text is not None else None


def functions(text):
    """{symbol: sha256 of its body and kernel descriptor, local labels without the function's ordinal}"""
    out = {}
    for m in re.finditer(r'^\t\.type\t(\S+),@function\n', text or '', re.M):
        name = m.group(1)
        body = text[m.end():text.index('\n', re.compile(r'^\.Lfunc_end\d+:', re.M).search(text, m.end()).start())]
        desc = re.search(r'^\t\.amdhsa_kernel ' + re.escape(name) + r'\n.*?^\t\.end_amdhsa_kernel\n', text, re.M | re.S)
        body = re.sub(r'\.L(BB|JTI|func_begin|func_end|tmp)\d+', r'.L\1', body + (desc.group(0) if desc else ''))
        body = re.sub(r'\bBB\d+_', 'BB_', body)          # (the same ordinal in the loop comments: "Header=BB9_14" ...
        body = re.sub(r'[ \t]+;', ' ;', body)            # ... which are padded to a column behind labels of either length)
        out[name] = sha(body)
    return out


rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD'
with tempfile.TemporaryDirectory() as tmp:
    out, old = os.environ.get('ISA_KEEP') or tmp, os.path.join(tmp, 'tree')
    os.makedirs(old)
    tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'piml_amd/csrc', 'include'], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
    names = sorted({os.path.basename(s) for s in B.sources()} | {f for f in os.listdir(os.path.join(old, 'piml_amd', 'csrc')) if f.endswith('.hip')})
    with ThreadPoolExecutor(int(os.environ.get('PIML_BUILD_JOBS', '4'))) as ex:
        rows = list(ex.map(lambda n: (n, asm(old, n, os.path.join(out, 'before')), asm(ROOT, n, os.path.join(out, 'after'))), names))
print(f'| file | sha256 at {rev} | sha256 of this tree | same |\n|---|---|---|---|')
for n, a, b in rows:
    print(f'| {n} | {sha(a)} | {sha(b)} | {"yes" if a == b else "NO"} |')
bad = False
for n, a, b in rows:
    if a == b:
        continue
    fa, fb = functions(a), functions(b)
    nice = {f: _demangle_lite(f) for f in set(fa) | set(fb)}
    print(f'\n{n}, function by function:\n\n| function | at {rev} | this tree | |\n|---|---|---|---|')
    for f in sorted(nice, key=nice.get):
        verdict = 'same' if fa.get(f) == fb.get(f) else 'only before' if f not in fb else 'only after' if f not in fa else 'DIFFERENT'
        bad = bad or verdict in ('only after', 'DIFFERENT')
        print(f'| `{nice[f]}` | {(fa.get(f) or "-")[:16]} | {(fb.get(f) or "-")[:16]} | {verdict} |')
sys.exit(bad)
