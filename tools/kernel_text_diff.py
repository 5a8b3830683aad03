"""Are the kernels of a source file the same in two trees?  For refactors of host code: compiles FILE device-only for gfx950 with
the flags of feddlib_amd/build.py in both trees and compares, kernel by kernel, the instruction text and the kernel descriptor
(the .amdhsa_kernel block).  Local labels carry the function's position in the module and are compared without it.

    python tools/kernel_text_diff.py OTHER_TREE spmv.hip assemble_tiles.hip

Prints one line per file (kernels here / there / identical) and the names that differ; exit status 1 if any does.  No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from feddlib_amd import build  # noqa: E402


def kernels(tree, name):
    src = os.path.join(tree, "feddlib_amd", "csrc", name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], check=True)
        text = open(out).read()
    text = re.sub(r"(?<![A-Za-z0-9_])(\.L)?BB\d+_", r"\1BB_", text)       # (labels and the comments that name them)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        sym = m.group(1)
        body = re.search(r"^%s:[^\n]*\n.*?^\.Lfunc_end:" % re.escape(sym), text, re.S | re.M)
        found[sym] = (body.group(0) if body else "") + "\n" + m.group(0)
    return found


def main(argv):
    other, files, bad = argv[0], argv[1:], 0
    for f in files:
        a, b = kernels(HERE, f), kernels(other, f)
        differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
        only = sorted(a.keys() ^ b.keys())
        print("%s: %d kernels here, %d there, %d identical" % (f, len(a), len(b), len(a.keys() & b.keys()) - len(differ)))
        for k in differ:
            print("  differs: " + k)
        for k in only:
            print("  only in one tree: " + k)
        bad += len(differ) + len(only)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
