"""The rules of setalleles_hip (vcfgl_amd/csrc/misc/sal_core.h: what the host path and the kernel run) on the CPU under AddressSanitizer
and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/sal_core_main.cpp), every text in a heap block of exactly
its length.
  1. the PL token parser against strtol (the program compares) and against the model's grammar
  2. the normalisations: the first-NaN rule for the missing pattern, end-of-vector and a real NaN at every place, a NaN the arithmetic
     makes, the PL sample of nothing but end-of-vector, the casts that would overflow
  3. the narrowing thresholds of htslib's integer writer
  4. BCF: a sample's old vector at every integer width and as floats, gathered and normalised; the narrowed values read back
  5. whole records of the generator, regions that end exactly at the block's end: status, column count and every plane value
Required: the model's result (tests/sal_file_model.py) and no sanitizer report."""
import os
import subprocess

import numpy as np
import pytest

import sal_file_model as M
import setal_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sal_core") / "sal_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "sal_core_main.cpp")]
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
    return got[:-1]


hx = lambda s: s.encode().hex() or "-"


def test_the_pl_token_parser_against_strtol(program, tmp_path):
    toks = [".", "0", "7", "-0", "+5", "-5", "255", "2147483647", "2147483648", "-2147483648", "-2147483649", "+2147483647", "0000000001",
            "00000000001", "9999999999", "-9999999999", "", "-", "+", "..", "1.", "1e1", " 1", "1 ", "12a", "a", "--1", "+-1", "1,2", "0x10"]
    rng = np.random.default_rng(2)
    toks += [str(int(v)) for v in rng.integers(-2 ** 31, 2 ** 31, size=300)] + [str(int(v)) for v in rng.integers(-300, 300, size=100)]
    got = run(program, tmp_path, ["P " + hx(t) for t in toks])
    assert not [(t, g) for t, g in zip(toks, got) if g.startswith("MISMATCH")]
    assert [g != "host" for g in got] == [M.pl_in_grammar(t) for t in toks]
    assert [int(g) for t, g in zip(toks, got) if g != "host"] == [M.pl_value(t) for t in toks if M.pl_in_grammar(t)]
    assert dict(zip(toks, got))["-2147483648"] == str(-2 ** 31) and dict(zip(toks, got))["00000000001"] == "host"


def f32(x):
    return int(np.float32(x).view(np.uint32))


def norm_cases():
    MISS, END, NAN, NEG = M.F_MISSING, M.F_END, 0x7FC00001, 0xFFC00000
    out = []
    base = [f32(-1.5), f32(-0.25), f32(-3), f32(0), f32(-7.125), f32(-2)]
    for bad in (MISS, END, NAN, NEG):
        for at in range(6):
            v = list(base); v[at] = bad
            out += [(0, v), (2, v)]
        out.append((0, [bad] * 3)); out.append((2, [END, bad, MISS]))
    out += [(0, base), (2, [f32(x) for x in (0.1, 0.2, 0.3, 0.4)]), (0, [f32(-np.inf)] * 3), (0, [f32(np.inf), f32(1)]), (2, [0, 0, 0]),
            (2, [f32(np.inf), f32(1), f32(2)]), (0, [f32(-0.0)]), (2, [f32(1e-45)] * 15), (0, [f32(-i) for i in range(15)])]
    I = lambda v: v & 0xFFFFFFFF
    out += [(1, [I(M.I_END)] * 3), (1, [I(M.I_END)] * 15), (1, [I(M.I_END), 5, 7]), (1, [5, I(M.I_END)]), (1, [I(M.I_MISSING), I(M.I_END), 9]),
            (1, [9, 3, I(M.I_MISSING)]), (1, [10, 3, 255]), (1, [I(-5), 3, 0]), (1, [I(-2000000000), 2000000000]), (1, [I(-2 ** 31 + 2), 0]),
            (1, [I(-2 ** 31 + 200), 0]), (1, [16777217, 0, 16777219]), (1, [I(M.I_END + 1), I(M.I_END + 1)]), (1, [2147483647, 0]), (1, [2147483647, I(-1)])]
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(1, 16))
        out.append((0, [f32(-x) for x in rng.random(n) * 30]))
        out.append((2, [f32(x) for x in rng.random(n)]))
        out.append((1, [int(x) for x in rng.integers(0, 70000, n)]))
    return out


def test_the_normalisations_and_the_first_nan_rule(program, tmp_path):
    cases = norm_cases()
    got = run(program, tmp_path, ["N %d %d %s" % (f, len(v), " ".join("%08x" % b for b in v)) for f, v in cases])
    n_over = 0
    for (f, v), g in zip(cases, got):
        a = np.array(v, np.uint32).reshape(-1, 1)
        if f == 1:
            want, over = M.norm_pl(a)
            n_over += over
            assert g == ("over" if over else " ".join("%08x" % b for b in want[:, 0])), (f, v)
        else:
            assert g == " ".join("%08x" % b for b in M.norm_float(a, f == 2)[:, 0]), (f, v)
    assert n_over == 6
    d = {(f, tuple(v)): g for (f, v), g in zip(cases, got)}
    E = M.I_END & 0xFFFFFFFF
    assert d[(1, (E, E, E))] == "00000000 00000000 00000000"                # nothing but end-of-vector: zeros
    assert d[(0, (f32(-np.inf),) * 3)] == "7fc00000 7fc00000 7fc00000"      # -inf - -inf: the canonical quiet NaN
    assert d[(2, (M.F_END, 0xFFC00000, M.F_MISSING))] == "7f800001 ffc00000 7f800001"   # the first NaN alone becomes the missing pattern


def test_the_narrowing_thresholds(program, tmp_path):
    cases = [(0, 127, 1), (0, 128, 2), (-120, 127, 1), (-121, 0, 2), (-121, 127, 2), (0, 32767, 2), (0, 32768, 4), (-32760, 32767, 2), (-32761, 0, 4),
             (0, 0, 1), (-2 ** 31 + 2, 0, 4), (0, 2 ** 31 - 1, 4)]
    assert run(program, tmp_path, ["W %d %d" % (a, b) for a, b, _ in cases]) == [str(w) for _, _, w in cases]


def test_whole_records_against_the_model(program, tmp_path):
    cases, want = [], []
    for N, seed, odd in [(1, 1, 0.0), (3, 2, 0.3), (7, 3, 0.0), (70, 4, 0.1)]:
        for tags in ("GL", "GL:PL", "GL:PL:GP"):
            for r in M.make_records(N, 12, seed, tags=tags, odd_share=odd, wide_pl=True):
                cols = [":".join(c[k] for k in r["keys"] if c[k] is not None) for c in r["cols"]]
                g2g = sm.genotype_map(sm.allele_map(r["alleles"], r["target"]))
                nGo, nGn = sm.n_gt(len(r["alleles"])), sm.n_gt(len(r["target"]))
                where = {t: r["keys"].index(t) for t in M.TAGS if t in r["keys"]}
                o2n = sum((h + 1) << (4 * g) for g, h in enumerate(g2g))
                k = [where.get(t, -1) for t in M.TAGS]
                cases.append("R %d %d %d %d %d %d %x %s" % (N, k[0], k[1], k[2], nGo, nGn, o2n, hx("\t".join(cols))))
                bad, stop, new = M.relabel_columns(r["keys"], where, cols, N, len(r["alleles"]), g2g, nGn)
                if bad:
                    want.append("1 %d" % N)
                elif stop:
                    want.append("2 %d" % N)
                else:
                    want.append("0 %d " % N + " ".join("%08x" % b for t in M.TAGS if t in where for b in new[t].reshape(-1)))
    # a column count other than N, more values than the old genotypes, a token outside the grammar beside both
    cases += ["R 2 0 -1 -1 3 3 321 " + hx("0,-1,-2"), "R 2 0 -1 -1 3 3 321 " + hx("0,-1,-2\t0,0,0\t0"), "R 1 0 -1 -1 3 3 321 " + hx("0,-1,-2,-3"),
              "R 1 0 -1 -1 3 3 321 " + hx("0,-1,-2x,-3"), "R 1 0 -1 -1 3 3 321 " + hx(""), "R 1 1 -1 -1 3 1 001 " + hx("5"), "R 1 0 -1 -1 3 3 421 " + hx("0")]
    want += ["2 1", "2 3", "2 1", "1 1", "1 1", "0 1 7f800001", "insane"]
    got = run(program, tmp_path, cases)
    assert [g.split()[0] for g in got].count("1") >= 5 and [g.split()[0] for g in got].count("0") >= 100
    assert got == want


def test_bcf_vectors_against_the_model(program, tmp_path):
    import struct
    rng = np.random.default_rng(5)
    cases, want = [], []
    for it in range(400):
        n_old = int(rng.integers(2, 6)); n_new = int(rng.integers(2, n_old + 1))
        old = list(range(n_old)); tgt = [int(a) for a in rng.permutation(n_old)[:n_new]]
        g2g = sm.genotype_map(sm.allele_map(old, tgt))
        nGo, nGn = sm.n_gt(n_old), sm.n_gt(n_new)
        n2o = [g2g.index(h) for h in range(nGn)]
        nib = sum((g + 1) << (4 * h) for h, g in enumerate(n2o))
        nv = int(rng.integers(1, nGo + 1)) if it % 4 == 0 else nGo
        f = it % 3
        if f == 1:
            ty = 1 + it % 3
            lim = (100, 30000, 2 ** 31 - 2)[ty - 1]
            vals = [None if u < 0.03 else "END" if u < 0.05 else int(x) for u, x in zip(rng.random(nv), rng.integers(-lim if it % 5 == 0 else 0, lim, nv))]
            data = M._ints(vals, ty)
            bits = M._bits_of([vals], nGo, True)
        else:
            ty = 5
            raw = [M.F_MISSING if u < 0.03 else M.F_END if u < 0.05 else 0x7FC00000 if u < 0.07 else f32(-x * 30 if f == 0 else x) for u, x in zip(rng.random(nv), rng.random(nv))]
            data = struct.pack("<%dI" % nv, *raw)
            bits = M._bits_of([raw], nGo, False)
        cases.append("B %d %d %d %d %x %s" % (f, ty, nv, nGn, nib, data.hex()))
        g = sm.scatter(bits, g2g, nGn, 0)
        if f == 1:
            out, over = M.norm_pl(g)
            want.append("over" if over else " ".join("%08x" % b for b in out[:, 0]))
        else:
            want.append(" ".join("%08x" % b for b in M.norm_float(g, f == 2)[:, 0]))
    got = run(program, tmp_path, cases)
    assert got == want and 5 <= want.count("over") <= 120
