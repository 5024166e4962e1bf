"""The per-sample rule of the BCF genotype decoder (vcfgl_amd/csrc/vgl_bcfin_core.h) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/bcfin_core_main.cpp) decodes every record of every case set
of tests/bcfin_cases.py from an allocation of exactly its slice into an allocation of exactly its row -- the eight-samples-a-step
path of int8 pairs and the one-sample path, slices at any address.  Required: the model's statuses, sums and rows, no sanitizer report."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bcfin_cases as bc
import bcfin_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bcfin_core") / "bcfin_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "bcfin_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def case_file(case, path):
    buf, begin, gt_type, n, nal, amap = case.arrays()
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", len(begin), case.N))
        for i in range(len(begin)):
            k = case.slice_bytes(i)
            f.write(struct.pack("<iii5bq", int(gt_type[i]), int(n[i]), int(nal[i]), *[int(x) for x in amap[i]], k))
            f.write(buf[int(begin[i]):int(begin[i]) + k])


def want_text(case):
    rows, sums, status = case.expected()
    return "".join("%d %d %s\n" % (0, sums[i], bytes(rows[i]).hex()) if status[i] == bm.BCFIN_OK else "1 - -\n" for i in range(len(status)))


@pytest.mark.parametrize("name", sorted(bc.all_cases()))
def test_the_core_equals_the_model(program, name, tmp_path):
    case = bc.all_cases()[name]
    path = str(tmp_path / "cases.bin")
    case_file(case, path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout == want_text(case)
    assert sum(l.startswith("1 ") for l in r.stdout.splitlines()) == len(case.fallback)


def test_records_the_five_entry_map_cannot_describe(program, tmp_path):
    """n_alleles 0 and 6: the caller's records, whatever their values"""
    c = bc.Case(9)
    vals = [[bc.gt_value(0), bc.gt_value(1, 1)]] * 9
    c.add(vals).add(vals, nal=6, fallback=True).add(vals, nal=0, fallback=True).add(vals, nal=5)
    path = str(tmp_path / "cases.bin")
    case_file(c, path)
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    assert [l.split()[0] for l in r.stdout.splitlines()] == ["0", "1", "1", "0"] and r.stdout == want_text(c)
