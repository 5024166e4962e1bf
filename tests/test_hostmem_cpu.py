"""The owners of the host library's device and pinned memory (vcfgl_amd/csrc/hostlib/mem.h: DevBuf, PinBuf, TextOut) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/hostmem_main.cpp) compiles the header
with -DVGL_MEM_TEST -- malloc / free with a "fail the k-th allocation" counter in place of the HIP allocator -- and covers growth,
the no-op reserve, reserve(0), a failure at each allocation index (buffer left empty, account exact), moves, the non-owning state
(never freed) and TextOut::reserve failing on its second and third buffers.  Required: every check of the program, the account back
at zero, and no report of the sanitizers (the leak checker included)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostmem") / "hostmem_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-DVGL_MEM_TEST", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostmem_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_owners_under_the_sanitizers(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "checks" and int(words[1]) >= 40
