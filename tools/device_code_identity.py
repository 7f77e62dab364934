"""Is the gfx950 device code of this tree the same as that of an earlier revision?  CPU only, no GPU needed.

    python tools/device_code_identity.py <parent-rev> [--keep DIR]

Writes <parent-rev>'s tante_amd/csrc, tante_amd/build.py and include/ into a temporary directory (git archive), compiles every entry
of build.SOURCES on both sides with --offload-device-only -c -- each side with the FLAGS + EXTRA_FLAGS of its OWN build.py, the same
relative source path and the same -cuid on both (hipcc otherwise derives the compilation unit's id, which goes into the names of
internal symbols, from the absolute path and the flags) -- and compares the sha256 of the two device objects.  One line per source;
exit status 1 if any differs.  --keep DIR leaves the objects in DIR (for llvm-objdump -d / tools/kernel_resources.py on a pair that differs)."""
import hashlib
import importlib.util
import io
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build(root):
    spec = importlib.util.spec_from_file_location("_build_" + hashlib.md5(root.encode()).hexdigest(), os.path.join(root, "tante_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_side(root, out, jobs=16):
    b = load_build(root)
    os.makedirs(out, exist_ok=True)

    def one(src):
        obj = os.path.join(out, src.replace(".hip", ".o"))
        cmd = [b.HIPCC, *b.FLAGS, *b.EXTRA_FLAGS.get(src, []), "--offload-device-only", "-cuid=" + src, "-c", os.path.join("tante_amd", "csrc", src), "-o", obj]
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed in {root}: {' '.join(cmd)}\n{r.stderr}")
        with open(obj, "rb") as f:
            return src, hashlib.sha256(f.read()).hexdigest()

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        return b, dict(ex.map(one, b.SOURCES))


def main():
    args = sys.argv[1:]
    keep = None
    if "--keep" in args:
        i = args.index("--keep")
        keep = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    if len(args) != 1:
        sys.exit(__doc__)
    rev = args[0]
    with tempfile.TemporaryDirectory() as tmp:
        work = keep or tmp
        parent = os.path.join(work, "parent")
        os.makedirs(parent, exist_ok=True)
        tar = subprocess.run(["git", "archive", rev, "tante_amd/csrc", "tante_amd/build.py", "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(parent)
        # the two sides share the 16 jobs
        with ThreadPoolExecutor(max_workers=2) as ex:
            fp = ex.submit(compile_side, parent, os.path.join(work, "obj_parent"), 8)
            ft = ex.submit(compile_side, ROOT, os.path.join(work, "obj_this"), 8)
            (bp, hp), (bt, ht) = fp.result(), ft.result()
    ver = subprocess.run([bt.HIPCC, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    print("hipcc: " + "; ".join(l for l in ver if "version" in l))
    print(f"parent: {subprocess.run(['git', 'rev-parse', '--short', rev], cwd=ROOT, capture_output=True, text=True).stdout.strip()}")
    print("| source | parent sha256 | this tree sha256 | |")
    print("|---|---|---|---|")
    bad = 0
    for src in bt.SOURCES:
        a, b = hp.get(src, "-"), ht[src]
        bad += a != b
        print(f"| {src} | {a[:16]} | {b[:16]} | {'identical' if a == b else 'DIFFERENT'} |")
    print(f"{len(bt.SOURCES) - bad} of {len(bt.SOURCES)} identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
