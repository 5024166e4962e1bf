"""The rules of fetchgl_hip (vcfgl_amd/csrc/misc/fgl_core.h: what the host path and the kernels run) on the CPU under AddressSanitizer
and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/fgl_core_main.cpp) parses tokens and records, each in a
heap block of exactly its length.
  1. the token parser against strtod and a cast (the program compares) and against Python's float (this file): every GL token of the
     golden VCFs, the %.6g / %.9g / %.15g texts of fetchgl_model.value_set(), ties of the double -> float rounding, both sides of the
     15-digit and |k| = 22 limits, and tokens that must be refused
  2. the column rule on regions that end exactly at the block's end
  3. the n_gls / END / RANGE rule
Required: the model's result (tests/fgl_file_model.py) and no sanitizer report."""
import glob
import os
import subprocess

import numpy as np
import pytest

import fetchgl_model as fm
import fgl_file_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fgl_core") / "fgl_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "fgl_core_main.cpp")]
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
    assert got[-1] == "" and len(got) == len(cases) + 1 and r.stdout.split()[:2] == ["cases", str(len(cases))]
    return got[:-1], r.stdout.split()


hx = lambda s: s.encode().hex() or "-"


def check_tokens(program, tmp_path, tokens):
    got, stdout = run(program, tmp_path, ["P " + hx(t) for t in tokens])
    assert not [(t, g) for t, g in zip(tokens, got) if g.startswith("MISMATCH")][:10]
    inside = [gm.in_grammar(t) for t in tokens]
    assert [g != "host" for g in got] == inside
    return got, inside


def golden_gl_tokens():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLD, "**", "*.vcf"), recursive=True)):
        for ln in open(path):
            f = ln.rstrip("\n").split("\t")
            if ln.startswith("#") or len(f) < 10 or "GL" not in f[8].split(":"):
                continue
            k = f[8].split(":").index("GL")
            for col in f[9:]:
                sub = col.split(":")
                if k < len(sub):
                    out += sub[k].split(",")
    return out


def test_every_gl_token_of_the_golden_files_is_inside_the_grammar(program, tmp_path):
    tokens = golden_gl_tokens()
    assert len(tokens) >= 4143 and tokens.count("-inf") >= 55
    got, inside = check_tokens(program, tmp_path, tokens)
    assert all(inside)
    for t, g in zip(tokens, got):
        assert g == "ok %08x" % (fm.MISSING_BITS if t == "." else gm.token_bits(t))


def test_the_decimal_texts_of_the_value_set(program, tmp_path):
    with np.errstate(invalid="ignore"):                                # (signalling NaN patterns)
        vals = fm.value_set().view(np.float32).astype(np.float64)
    tokens = [fmt % v for fmt in ("%.6g", "%.9g", "%.15g") for v in vals]
    got, inside = check_tokens(program, tmp_path, tokens)
    assert sum(inside) > len(tokens) // 3 and inside.count(False) > 1000          # both outcomes, by the hundred thousand
    # %.9g gives a float32 back: the parser's float is the value itself wherever the text is inside the grammar
    n = len(vals)
    bits = fm.value_set()
    for i in range(0, n, 7):
        g = got[n + i]
        if g != "host" and vals[i] == vals[i]:
            assert int(g.split()[1], 16) == int(bits[i]) or vals[i] == 0


TIES = ["16777217", "16777219", "16777217.0", "1.6777217e7", "167772170e-1", "16777217.000001", "16777216.999999", "-16777217", "+16777219",
        "33554434", "33554438", "1073741888", "1073741887.99999", "1073741888.00001", "0.000030517580863", "2.5", "0.1", "1e-5", "3.4028235e37"]
LIMITS = ["123456789012345", "1234567890123456", "0.123456789012345", "0.1234567890123456", "000123456789012345", "0001234567890123456", "123456789012345000",
          "1e22", "1e23", "1e-22", "1e-23", "0.0000000000000000000001", "0.00000000000000000000001", "123456789012345e22", "123456789012345e23", "1.5e-21", "1.5e-22",
          "12345.67890e+17", "12345.67890e+18", "1e999", "1e1000", "0e0", "-0", "-0.0e-5", "0e23", "1.", ".5", "-.5e1", "+1.e1", "00", "1e+05", "1E-05"]
REFUSED = ["", "+", "-", "+.", "-.", "e5", ".e5", "1e", "1e+", "1e-", "1e5x", "1..2", "1.2.3", "INF", "Inf", "infinity", "+inf", "-nan", "+nan", "NaN", "nan(1)", "0x10",
           "0x1p3", " 1", "1 ", "\t1", "--1", "+-1", "1e0001", "1e1.5", "1,2", "1:2", "..", "-", "1f", "1d5", "١"]


def test_ties_limits_and_refusals(program, tmp_path):
    tokens = TIES + LIMITS + REFUSED + [".", "inf", "-inf", "nan"]
    got, inside = check_tokens(program, tmp_path, tokens)
    want = dict(zip(tokens, got))
    assert want["16777217"] == "ok 4b800000" and want["16777219"] == "ok 4b800002" and want["16777217.000001"] == "ok 4b800001"   # ties to even
    assert want["1234567890123456"] == "host" and want["123456789012345"].startswith("ok") and want["000123456789012345"].startswith("ok")
    assert want["1e22"].startswith("ok") and want["1e23"] == "host" and want["1e-22"].startswith("ok") and want["1e-23"] == "host"
    assert want["123456789012345e22"].startswith("ok") and want["123456789012345e23"] == "host"
    assert want["-0"] == "ok 80000000" and want["."] == "ok 7f800001" and want["inf"] == "ok 7f800000" and want["-inf"] == "ok ff800000" and want["nan"] == "ok 7fc00000"
    assert all(want[t] == "host" for t in REFUSED)
    for t in TIES + LIMITS:
        if want[t] != "host":
            assert want[t] == "ok %08x" % gm.token_bits(t), t


def record_model(n, k, g, text):
    cols = text.split("\t")
    fields = []
    for col in cols:
        sub = col.split(":")
        fields.append(sub[k].split(",") if k < len(sub) else ["."])
    if any(g < len(t) and not gm.in_grammar(t[g]) for t in fields[:n]):
        return "host"
    n_gls = max(len(t) for t in fields[:n])
    if len(cols) != n or g >= n_gls:
        return "range %d" % n_gls
    bits = [fm.END_BITS if g >= len(t) else fm.MISSING_BITS if t[g] == "." else gm.token_bits(t[g]) for t in fields]
    return "ok %d " % n_gls + " ".join("%08x" % b for b in bits)


def test_records_in_regions_of_exactly_their_length(program, tmp_path):
    columns = ["0/0:-1,-2.5,-3e1", "0/1:-4,.,inf", "./.:.", "./.", "1/1:-7", "0/1:-1,-2", "0/0:,", "0/0::5", "0/0:-1,-2,-3,-4,-5,-6", "0/0:1e400,2,3", "0/0:1,2x,3",
               "0/0:nan,-inf,+5", "", ":", ":,,"]
    rows = []
    for n in (1, 2, 3, 5):
        for i in range(len(columns)):
            cols = [columns[(i + 3 * s) % len(columns)] for s in range(n)]
            for text in ("\t".join(cols), "\t".join(cols + ["0/0:9,9,9"]), "\t".join(cols[:-1]), "\t".join(cols) + "\t"):
                for g in (0, 1, 2, 3, 5, 6):
                    rows.append((n, 1, g, text))
                    rows.append((n, 1, g, text[:-1]))                  # the region cut one byte short
    gl_first = "-1,-2,-3:0/0\t.:0/1\t-4,-5\t-6,-7,1e-30:1/1"
    rows += [(4, 0, g, gl_first) for g in range(4)] + [(4, 2, g, "0/0:5:-1,-2\t0/0:5\t0/0\t0/0:5:-3") for g in range(3)]
    rows += [(65, 1, g, "\t".join("0/1:%d,%d.5" % (s, -s) for s in range(65))) for g in (0, 1, 2)]
    want = [record_model(*r) for r in rows]
    got, _ = run(program, tmp_path, ["R %d %d %d %s" % (n, k, g, hx(text)) for n, k, g, text in rows])
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    kinds = [w.split()[0] for w in want]
    assert kinds.count("host") > 20 and kinds.count("range") > 100 and kinds.count("ok") > 100
    assert any("7f800002" in w for w in want) and any("7f800001" in w for w in want)       # END and MISSING are reached


def test_every_value_into_an_allocation_of_its_planned_size(program, tmp_path):
    bits = [int(b) for b in fm.value_set(n_random=2000)]
    got, stdout = run(program, tmp_path, ["V %x" % b for b in bits])
    assert got == [fm.fmt_value_bits(b, fm.FLOAT) for b in bits]
    assert int(stdout[5]) == 48                                    # -FLT_MAX: the sign, 39 digits, ".000000" and the separator: fgl::VALUE_BOUND
