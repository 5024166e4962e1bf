"""The rules of the resident BCF walk (vcfgl_amd/csrc/misc/rb_core.h: what the kernels of resident_file.hip run for --resident-bcf 1)
on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/rb_core_main.cpp),
every file in a heap block of exactly its length.

Sound files (fgl_file_model.bcf_bytes: 1, 3 and 65 samples, drawn and fixed alleles, every FORMAT mix of the generator, vectors of
fifteen values with their extended length): the host model of the passes, at 1, 2, 7 and 2^20 records a chain launch and at windows of
32, 48 and RB_WINDOW bytes, must give the record offsets, the heads and the field table of a soft cursor's walk and flag nothing, and
the host routines (bcf_shared, bcf_format_fields) must read from the heads what they read from the file.
Damaged files (every truncation of a small file, a few thousand single-byte changes of head bytes): the model flags wherever the
cursor fails; where the cursor does not fail, the model agrees with it or flags.
Required: `ok` for every case and no sanitizer report."""
import os
import subprocess

import pytest

import fgl_file_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rb_core") / "rb_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "rb_core_main.cpp"), "-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(program, tmp_path, cases):
    fin, fout = str(tmp_path / "cases.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write("".join(c + "\n" for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = open(fout).read().split("\n")
    assert got[-1] == "" and len(got) == len(cases) + 1 and r.stdout.split() == ["cases", str(len(cases))]
    return got[:-1]


def sound_files():
    """name -> (bytes, records)"""
    out = {}
    for n in (1, 3, 65):
        out["drawn_%d" % n] = (gm.bcf_bytes(gm.make_records(n, 24, seed=40 + n), n), 24)
        out["fixed_%d" % n] = (gm.bcf_bytes(gm.make_records(n, 9, seed=50 + n, fixed_alleles=True), n), 9)
        for k, fmt in enumerate(gm.FORMATS):
            out["fmt_%d_%d" % (n, k)] = (gm.bcf_bytes(gm.make_records(n, 3, seed=60 + k, fmt=fmt), n), 3)
    out["no_record"] = (gm.bcf_bytes([], 3), 0)
    return out


def test_sound_files(program, tmp_path):
    files = sound_files()
    got = run(program, tmp_path, ["F " + data.hex() for data, _ in files.values()])
    res = dict(zip(files, got))
    assert all(g.startswith("ok ") for g in got), res
    for name, (_, records) in files.items():
        assert int(res[name].split()[1]) == records, (name, res[name])
    for n in (1, 3, 65):
        _, _, fields, fifteen, residues = res["fixed_%d" % n].split()
        assert int(fifteen) >= 9                                        # a record of five alleles carries fifteen GLs: 0xF5 0x11 0x0F
    seen = 0
    for g in got:
        seen |= int(g.split()[4])
    assert seen == 15                                                   # the GL blocks begin at all four residues mod 4


def test_truncations(program, tmp_path):
    data = gm.bcf_bytes(gm.make_records(3, 4, seed=7, fixed_alleles=True), 3)
    got = run(program, tmp_path, ["T " + data.hex()])
    assert got[0].startswith("ok "), got
    files, flagged, failed = (int(x) for x in got[0].split()[1:])
    assert files > 500 and flagged == failed and failed >= files - 5    # only a cut between two records leaves a sound file


def test_single_byte_changes(program, tmp_path):
    cases = []
    for n, seed in ((1, 11), (3, 12), (65, 13)):
        for fixed in (False, True):
            data = gm.bcf_bytes(gm.make_records(n, 6, seed=seed, fixed_alleles=fixed), n)
            cases.append("M %d 600 %s" % (seed, data.hex()))
    got = run(program, tmp_path, cases)
    assert all(g.startswith("ok ") for g in got), got
    files, flagged, failed = (sum(int(g.split()[k]) for g in got) for k in (1, 2, 3))
    assert files == 3600 and flagged > 500 and failed > 200 and flagged >= failed and flagged < files
