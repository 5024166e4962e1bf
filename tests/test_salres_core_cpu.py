"""The rules by which setalleles_hip --resident 1 assembles its output records (vcfgl_amd/csrc/misc/salres_core.h: what k_salres_plan and
k_salres_write run) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main
(tests/salres_core_main.cpp).
  1. whole records of the generator (tests/sal_file_model.py: every tag set, DP first, an untouched field between the tags, AD last, and
     a record with no FORMAT at all): the piece table built from the record's head, the planned length and the bytes the host model of
     k_salres_write makes against the bytes put_record_bcf makes (setalleles_hip --on-device 0 -O u), with the output and the file at
     all 16 residues mod 16.  The file lives in a heap block of exactly its length and its last record ends at the block's last byte,
     so a read past `total` is a sanitizer report
  2. copy_run with source and destination at all 16 residues and runs of 0, 1, 15, 16, 17 and 4099 bytes
Required: equal bytes and no sanitizer report."""
import os
import subprocess

import pytest

import sal_file_model as M
from vcfgl_amd import setalleles as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("salres_core") / "salres_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "salres_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(program, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
    return r.stdout.split()


@pytest.mark.parametrize("tags", M.TAG_SETS)
@pytest.mark.parametrize("N", [1, 5, 67])
def test_whole_records_against_put_record_bcf(program, tmp_path, tags, N):
    recs = M.make_records(N, 10, seed=11 + N, tags=tags, wide_pl=True)
    brecs = M.bcf_records(recs, N, end_every=4)
    brecs[3]["fmt"] = []                                               # a record with no FORMAT at all
    path, tsv, out = str(tmp_path / "in.bcf"), str(tmp_path / "in.tsv"), str(tmp_path / "want")
    M.write_bcf(path, brecs, N, "bcf")
    open(tsv, "w").write(M.tsv_text(recs))
    rc, _, se = S.set_file(path, tsv, out, "u", on_device=False, timeout=120)
    assert rc == 0, se[-2000:]
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    assert M.read_bcf(out + ".bcf")[1] == want.records                 # (the host path is the model's: what the pieces are held against)
    if tags == "GL:PL:GP":
        assert {t for r in want.records for k, t, per in r["fmt"] if k == "PL"} == {1, 2, 3}      # every PL width
    got = run(program, "records", path, out + ".bcf", N, M.BCF_DICT["GL"], M.BCF_DICT["PL"], M.BCF_DICT["GP"])
    n_tags = len([t for t in tags.split(":") if t])
    assert got == ["ok", str(16 * 3 * 10), "records", "10", "touched", str(9 * n_tags)]


def test_copy_runs_at_every_residue_and_length(program):
    assert run(program, "runs") == ["ok", str(6 * 16 * 16 * 2 * 3)]
