"""No-GPU checks of the device pileup formatter's surroundings: the Python model re-renders the reference's golden pileups byte for
byte, the C ABI declares and binds the new entry points, the bound's host arithmetic, and the host program's refusals of
--device-pileup."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as gu
import pileup_model as pm
from vcfgl_amd import _abi, pileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
DOC = os.path.join(ROOT, "tests", "golden", "doc_error_qs")
ENTRIES = ["vgl_pileup_bound", "vgl_pileup_workspace_bytes", "vgl_pileup_format_device", "vgl_ctx_pileup_bound", "vgl_ctx_pileup_next"]
GOLDEN = ["test10", "error_qs0", "error_qs1", "error_qs2"]


def golden_text(name):
    if name == "test10":
        return gzip.open(os.path.join(gu.REFVCF, "reference", "test10", "test10.pileup.gz"), "rt").read()
    return open(os.path.join(DOC, name + ".pileup")).read()


@pytest.mark.parametrize("name", GOLDEN)
def test_model_rerenders_the_golden_pileups(name):
    text = golden_text(name)
    rows = pm.parse_lines(text)
    if name == "test10":
        assert rows == gu.read_pileup(os.path.join(gu.REFVCF, "reference", "test10", "test10.pileup.gz"))
    dp, reads = pm.arrays_of(rows)
    assert (dp == 0).any() and (dp > 0).any()
    body, off = pm.render(np.zeros(len(rows), np.int32), dp, reads)
    prefixes = [b"%s\t%d\t%s" % (c.encode(), p, r.encode()) for c, p, r, _ in rows]
    assert b"".join(pre + body[off[i]:off[i + 1]] for i, pre in enumerate(prefixes)) == text.encode()
    # an empty site has no text, every other status keeps its line
    st = np.array([(-3, pm.SITE_SKIP_EMPTY, 0, 1)[i % 4] for i in range(len(rows))], np.int32)
    b2, o2 = pm.render(st, dp, reads)
    assert all((o2[i + 1] == o2[i]) == (st[i] == pm.SITE_SKIP_EMPTY) for i in range(len(rows)))
    assert b2 == b"".join(body[off[i]:off[i + 1]] for i in range(len(rows)) if st[i] != pm.SITE_SKIP_EMPTY)


def test_model_quality_rules():
    reads = np.array([[[0b101110]], [[0b11]]], np.uint8)           # score 11 base G, score 0 base T
    dp = np.array([[2]], np.int32)
    assert pm.render([0], dp, reads)[0] == b"\t2\tGT\t,!\n"
    assert pm.render([0], dp, reads, qual=ord("5"))[0] == b"\t2\tGT\t55\n"
    assert pm.render([0], dp, reads, qual=np.array([[[-1]], [[63]]]))[0] == b"\t2\tGT\t `\n"
    assert pm.render([0], np.array([[0]], np.int32), reads)[0] == b"\t0\t*\t*\n"
    assert pm.adjusted_score(0.0) == -1 and pm.adjusted_score(1.0) == -1 and pm.adjusted_score(1e-9) == 63
    assert pm.adjusted_score(0.01) == 20 and pm.adjusted_score(0.0125) == 19 and pm.adjusted_score(0.0125, bins=[(0, 20, 7), (21, 63, 30)]) == 7


def test_header_declares_the_pileup_entries():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define VGL_ABI_VERSION 7\b", hdr) and _abi.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(r"VGL_API\s+\w+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    lib = _abi.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
    assert callable(pileup.format_columns) and callable(pileup.format_into)


def test_tile_struct_layout_matches_the_header(tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    assert cc, "no C compiler"
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "vcfgl_hip.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(vgl_pileup_tile));']
    src += [f'printf("{f} %zu\\n", offsetof(vgl_pileup_tile, {f}));' for f, _ in _abi.PileupTile._fields_]
    src.append("return 0; }")
    c_file, exe = tmp_path / "layout.c", tmp_path / "layout"
    c_file.write_text("\n".join(src) + "\n")
    lang = ["-x", "c"] if not cc.endswith("hipcc") else ["-x", "c++"]
    subprocess.run([cc] + lang + [str(c_file), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_abi.PileupTile)
    for f, _ in _abi.PileupTile._fields_:
        assert int(got[f]) == getattr(_abi.PileupTile, f).offset, f


def test_bound_host_arithmetic():
    lib = _abi.load_library()
    for N, S, R in [(1, 1, 0), (1, 1, 1), (3, 7, 9), (1000, 66, 72), (2500, 3, 100), (5, 4, 1020), (0, 5, 10), (7, 0, 10)]:
        want = S * (1 + N * pm.column_bound(R))
        assert lib.vgl_pileup_bound(N, S, R) == want == pileup.bound(N, S, R), (N, S, R)
    for R in range(0, 1100):                                     # every digit boundary: the longest column is that of dp = R (or dp = 0)
        assert pm.column_bound(R) == max(len(pm.column(d, np.zeros(max(d, 1), np.uint8))) for d in {0, R, max(R - 1, 0)}), R
    assert lib.vgl_pileup_bound(-1, 1, 1) == -1 and lib.vgl_pileup_bound(1, -1, 1) == -1 and lib.vgl_pileup_bound(1, 1, -1) == -1
    assert lib.vgl_pileup_workspace_bytes(3, 10) >= 4 * 30 and lib.vgl_pileup_workspace_bytes(-1, 10) == -1
    assert lib.vgl_ctx_pileup_bound(None, 10) == -1 and lib.vgl_ctx_pileup_next(None, None) == _abi.VGL_E_ARG


# (argv, what the message says besides the flag)
REFUSED = {
    "bad value": (["--device-pileup", "2", "-printPileup", "1"], "Allowed range is [0,1]"),
    "negative value": (["--device-pileup", "-1", "-printPileup", "1"], "Allowed range is [0,1]"),
    "no pileup": (["--device-pileup", "1"], "-printPileup 1"),
    "pileup off": (["--device-pileup", "1", "-printPileup", "0"], "-printPileup 1"),
    "depth inf": (["--device-pileup", "1", "-printPileup", "1", "--depth", "inf"], "--depth inf"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refuses_device_pileup_where_it_cannot_apply(case, tmp_path):
    assert os.path.exists(BIN), "vcfgl_hip not built"
    flags, why = REFUSED[case]
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", str(tmp_path / "o"), "--seed", "1", "-e", "0.01", "-O", "v"] + flags
    if "--depth" not in argv:
        argv += ["--depth", "2"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert "--device-pileup" in r.stderr and why in r.stderr and "Unknown argument" not in r.stderr
    assert not os.listdir(str(tmp_path))                       # refused before anything is written


def test_usage_lists_the_flag():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert "--device-pileup 0|1" in r.stdout + r.stderr
