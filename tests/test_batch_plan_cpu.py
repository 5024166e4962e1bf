"""The batch cutter of the misc programs (vcfgl_amd/csrc/misc/batch_plan.h: plan_batches, which fetchgl_hip, setalleles_hip and
gtdiscordance_hip call with their 64 MiB caps) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
with its own main (tests/batch_plan_main.cpp) runs it over 4500 random item lists with zero, one and two caps of 1 .. 64 -- an item
that alone exceeds a cap and an empty list among them -- and checks that the ranges partition the items in order with none empty or
above max_recs, that a batch of several items is within every cap, that no batch could have taken its successor's first item, that
the reported maxima are the batches' maxima, and that the ranges and maxima equal those of the two loops the programs carried before
the function existed.  Required: exit status 0, no report of the sanitizers and all of the program's checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
N_CASES = 3 * 1502 + 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "batch_plan_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plans_under_the_sanitizers(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    assert words[0] == "checks" and int(words[1]) >= 20 * N_CASES and words[2] == "cases" and int(words[3]) == N_CASES
