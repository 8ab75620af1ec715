"""Compare the gfx950 device code of csrc/kernels/*.hip between two source trees, kernel by kernel.

    python tools/isa_diff.py OTHER_REPO_ROOT attention.hip decode_fused.hip rope_cache.hip

Each file is compiled in both trees with the build's HIP_FLAGS to device assembly.  The assembly is
split per kernel, comments are dropped, and symbol names and the function index of local labels
are replaced by placeholders, so a kernel that was only renamed or moved compares equal.  The two
multisets of kernel bodies are compared; for a kernel on one side only, the resource-usage remarks
(registers, scratch, occupancy, LDS) are printed.  Exit status 1 if any file differs.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from polykey_service_amd._native.build import HIP_FLAGS, HIPCC  # noqa: E402


def compile_asm(root: str, fname: str, out: str):
    cmd = [HIPCC, "-x", "hip", *HIP_FLAGS, "-I" + os.path.join(root, "csrc"), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(root, "csrc", "kernels", fname), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise SystemExit(r.stdout)
    return open(out).read(), r.stdout


def kernels(asm: str) -> dict:
    """name -> normalised body of every kernel (.amdhsa_kernel symbols) in the assembly."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    bodies = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), asm, re.M | re.S)
        lines = []
        for line in m.group(1).splitlines():
            line = re.sub(r"\s*;.*", "", line).strip()            # comments
            line = re.sub(r"\.LBB\d+_", ".LBBN_", line)           # function index of local labels
            line = re.sub(r"_Z\w+", "SYM", line)                  # mangled names (kernel, LDS, callees)
            if line:
                lines.append(line)
        bodies[name] = "\n".join(lines)
    return bodies


def remarks(log: str) -> dict:
    """kernel name -> its resource-usage remark lines."""
    out, cur = collections.defaultdict(list), None
    for line in log.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = f.group(1)
        elif cur:
            out[cur].append(m.group(1).strip())
    return out


def main() -> int:
    other, files = sys.argv[1], sys.argv[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for fname in files:
            a_asm, a_log = compile_asm(other, fname, os.path.join(tmp, "a.s"))
            b_asm, b_log = compile_asm(REPO, fname, os.path.join(tmp, "b.s"))
            a, b = kernels(a_asm), kernels(b_asm)
            ca, cb = collections.Counter(a.values()), collections.Counter(b.values())
            same = ca == cb
            print(f"{fname}: {len(a)} kernels there, {len(b)} here: {'identical' if same else 'DIFFERENT'}")
            if same:
                continue
            bad = 1
            for side, ks, mine, theirs, log in (("there", a, ca, cb, a_log), ("here", b, cb, ca, b_log)):
                rem = remarks(log)
                for name, body in ks.items():
                    if mine[body] > theirs[body]:
                        print(f"  only {side}: {name}\n    " + "; ".join(rem.get(name, [])))
    return bad


if __name__ == "__main__":
    sys.exit(main())
