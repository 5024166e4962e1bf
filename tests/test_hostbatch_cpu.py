"""The pure layer of the host batches (vcfgl_amd/csrc/hostlib/batch.h: the staging layouts of vgl_vcfin / bcfin / inflate _host_*, the
two-slot ring, the stream handle's tickets, every family's buffers as owners) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/hostbatch_main.cpp) compiles the header with
-DVGL_MEM_TEST, as tests/test_hostmem_cpu.py does for mem.h.  It covers: every section offset and both used sizes of the three
layout functions against the formulas the handles' create and submit used to carry separately (counts 0, 1, counts whose L * 4 and
L * 5 are no multiples of 256, the maxima), used <= capacity <= the former capacity; tickets 0, 1, 0, ..., the third batch refused
with the "in flight" text, tickets -1, 2 and a ticket that is not busy refused; the stream handle's "submit order" and "bad ticket"
refusals; an allocation failure at every index of every family's buffers with no block left.  Required: exit status 0, no report
of the sanitizers (the leak checker included) and all of the program's checks -- a full run counts 1496."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
N_CHECKS = 1496


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostbatch") / "hostbatch_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-DVGL_MEM_TEST", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostbatch_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_layouts_rings_and_failures_under_the_sanitizers(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "checks" and int(words[1]) >= N_CHECKS
