"""BlockManager.fork: the stand-alone host test program (csrc/tests/test_fork.cpp: 1,000 random fork /
free / allocate / commit / match operations under the ref-count and pool invariants, fork-failure
atomicity) built with AddressSanitizer + UndefinedBehaviorSanitizer and run directly on the CPU, and
the pybind11 face of the same call."""
import os
import subprocess

from polykey_service_amd._native.loader import load_extension

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_fork_core_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_fork")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "csrc", "tests", "test_fork.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fork tests OK" in r.stdout


def test_fork_python_face():
    bm = load_extension("_pk_runtime").BlockManager(8, 32, 0, True)
    assert bm.allocate(1, 71)
    src = bm.table(1)
    pairs = bm.fork(1, 2, 70)
    dst = bm.table(2)
    assert dst[:2] == src[:2] and dst[2] != src[2] and pairs == [(src[2], dst[2])]
    assert [bm.ref_count(b) for b in src] == [2, 2, 1]
    assert bm.fork(1, 3, 64) == [] and bm.table(3) == src[:2]
    free = bm.num_free
    assert bm.fork(1, 2, 70) is None and bm.fork(5, 6, 8) is None and bm.fork(1, 6, 97) is None
    assert bm.num_free == free and not bm.has(6)
    for s in (1, 2, 3):
        bm.free_seq(s)
    assert bm.num_free == 8 and bm.num_seqs == 0
