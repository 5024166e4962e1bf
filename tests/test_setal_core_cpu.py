"""The set-alleles maps and per-sample routines (vcfgl_amd/csrc/vgl_setal_core.h) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/setal_core_main.cpp) runs every (old list, target list) of
2 .. 5 distinct alleles in every order through the header and through a second, straightforward implementation, with missing samples,
-inf entries, one-byte PL 255 and a GP sum whose float order matters.  Required: no difference and no sanitizer report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("setal_core") / "setal_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "setal_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_map_and_the_special_samples(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # ordered selections of 2 .. 5 out of 5 alleles: (20 + 60 + 120 + 120)^2 pairs; a target is accepted iff it is a subset of the record's
    # alleles: sum over old counts n of P(5, n) * sum_{m <= n} P(n, m) = 40 + 720 + 7200 + 38400; 14 samples per accepted pair
    assert r.stdout.split() == ["pairs", "102400", "subsets", "46360", "refused", "56040", "samples", str(46360 * 14)]
