"""The fetch-GL formatter (vcfgl_amd/csrc/vgl_fetchgl_core.h) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program with its own main (tests/fetchgl_core_main.cpp) formats the value set in both value modes, each value into an
allocation of exactly the size its counting pass gave.  Required: the model's text for every value and no sanitizer report."""
import os
import subprocess

import pytest

import fetchgl_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fetchgl_core") / "fetchgl_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "fetchgl_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_value_of_the_set_in_both_modes(program, tmp_path):
    pats = fm.value_set()
    assert len(pats) > 100000
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    pats.tofile(fin)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.split() == ["values", str(len(pats)), "longest", "47", "genotypes", "55"]
    got = open(fout).read().split("\n")
    assert got[-1] == "" and len(got) == 2 * len(pats) + 1
    for mode in (fm.FLOAT, fm.TEXT):
        bad = [(hex(int(b)), g, fm.fmt_value_bits(b, mode)) for b, g in zip(pats, got[mode * len(pats):(mode + 1) * len(pats)])
               if g != fm.fmt_value_bits(b, mode)]
        assert not bad, (mode, len(bad), bad[:10])
