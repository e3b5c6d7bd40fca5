"""Device-code identity check for host-side refactors: compiles each given csrc/*.hip of a tree device-only for gfx950 (the flags
of __graft_entry__.build) and prints, per file, the kernel count and the sha1 of the code object's .text (instructions),
.rodata (kernel descriptors) and .note (registers, spills, LDS, arguments). Run it on two trees: equal lines = the same kernels.
Whole code objects differ between any two source texts (.dynsym carries an id derived from the text), hence the sections.

    python scripts/codeobj_sections.py TREE_ROOT gemm_bf16.hip gemm_bf16_256.hip ..."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import FLAGS, HIPCC  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def tool(name):
    llvm = [os.path.join(os.path.dirname(os.path.realpath(HIPCC)), *rel) for rel in (("..", "lib", "llvm", "bin"), ("..", "llvm", "bin"))]
    path = shutil.which(name) or shutil.which(name, path=os.pathsep.join(llvm))
    if not path:
        raise SystemExit(f"{name} not found (looked on PATH and beside {HIPCC})")
    return path


def sections(root, hip, tmp):
    csrc = os.path.join(root, "cvml_goalnet_amd", "csrc")
    co = os.path.join(tmp, hip + ".co")
    subprocess.check_call([HIPCC, *FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-c", hip, "-o", co], cwd=csrc)
    syms = subprocess.check_output([tool("llvm-readelf"), "--dyn-syms", "--wide", co], text=True)
    kernels = sum(1 for line in syms.splitlines() if line.endswith(".kd"))        # one kernel descriptor per kernel
    out = [f"{kernels:3d} kernels"]
    for sec in SECTIONS:
        dump = os.path.join(tmp, hip + sec)
        subprocess.check_call([tool("llvm-objcopy"), f"--dump-section={sec}={dump}", co])
        with open(dump, "rb") as f:
            out.append(f"{sec} {hashlib.sha1(f.read()).hexdigest()}")
    return "  ".join(out)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for hip in sys.argv[2:]:
            print(f"{hip:20s} {sections(os.path.abspath(sys.argv[1]), hip, tmp)}", flush=True)
