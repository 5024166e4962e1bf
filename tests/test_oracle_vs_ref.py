"""Checks the oracle's samplers and tables against the reference's OWN code: rng.h + shared.cpp compiled from the reference
checkout into oracle/_ref by oracle/Makefile, their outputs on the inputs below stored in tests/golden/ref_samplers.json by
oracle/ref_vectors.py (sha256 of every sequence + its first values).  The oracle's sequences must hash to the same values."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ref_samplers.json")) as fh:
    REF = json.load(fh)


def _same(got, want):
    """`got` (the oracle) equals the reference's sequence `want` value for value"""
    got = np.ascontiguousarray(got)
    got = got.astype(got.dtype.newbyteorder("<"))
    assert got.dtype.str == want["dtype"] and got.size == want["n"], (got.dtype.str, got.size)
    assert got.ravel()[:len(want["head"])].tolist() == want["head"]
    return hashlib.sha256(got.tobytes()).hexdigest() == want["sha256"]


@pytest.mark.parametrize("seed", [42, 0, -1, 123456789, -7, 2 ** 31 - 1])
def test_rand48_streams(oracle, seed):
    """glibc drand48/erand48 == closed-form LCG; all three reference streams start equal."""
    o = oracle.lib()
    x = o.vgl_oracle_rand48_seed(seed)
    u = np.zeros(2000)
    for i in range(2000):
        x = o.vgl_oracle_rand48_jump(x, 1)
        u[i] = x / 2.0 ** 48
    rng0, rng1, rng2 = REF["rand48"][str(seed)]
    assert _same(u, rng0) and _same(u, rng1) and _same(u, rng2)


def test_rand48_jump(oracle):
    o = oracle.lib()
    x0 = o.vgl_oracle_rand48_seed(42)
    x = x0
    for i in range(1, 5000):
        x = o.vgl_oracle_rand48_jump(x, 1)
        if i % 97 == 0:
            assert x == o.vgl_oracle_rand48_jump(x0, i)
    big = 3 * 2 ** 40 + 12345
    assert o.vgl_oracle_rand48_jump(o.vgl_oracle_rand48_jump(x0, big), 2 ** 48 - big) == x0  # full period


def test_gamma_ln(oracle):
    o = oracle.lib()
    assert _same(np.array([o.vgl_oracle_gamma_ln(v) for v in np.linspace(0.5, 700, 20000)]), REF["gamma_ln"])


def test_qscore_lut_all_entries(oracle):
    """shared.cpp:110-114 (3 x 257 seven-digit literals) == the oracle's regenerated table."""
    o = oracle.lib()
    assert _same(np.array([[o.vgl_oracle_q2gl(row, q) for q in range(257)] for row in range(3)]), REF["q2log10gl"])


@pytest.mark.parametrize("lam", [0, 0.1, 2, 5, 10, 11.99, 12, 20, 30, 100, 499.5])
def test_poisson(oracle, lam):
    o = oracle.lib()
    n = 20000
    b = np.zeros(n, np.int32)
    st = C.c_uint64(o.vgl_oracle_rand48_seed(42))
    o.vgl_oracle_poisson_draws(lam, C.byref(st), n, b.ctypes.data)
    want = REF["poisson"][repr(lam)]
    assert _same(b, want)
    if lam == 100:
        assert want["head"][0] == 85          # DP of the first record of test/reference/test18


@pytest.mark.parametrize("mv", [(0.01, 1e-5), (0.024, 1e-5), (0.4, 0.1), (0.2, 0.1), (0.001, 1e-7)])
def test_beta_samplers(oracle, mv):
    m, v = mv
    o = oracle.lib()
    n = 20000
    b = np.zeros(n)
    o.vgl_oracle_beta_std_draws(m, v, 42, n, b.ctypes.data)
    assert _same(b, REF["beta_std"][repr(mv)]), "std::mt19937 / std::gamma_distribution restatement"
    st = C.c_uint64(o.vgl_oracle_rand48_seed(42))
    o.vgl_oracle_beta_rand48_draws(m, v, C.byref(st), n, b.ctypes.data)
    assert _same(b, REF["beta_rand48"][repr(mv)]), "rand48 beta (reference built with -D__USE_STD_BETA__=0)"


def test_doc_known_answers(oracle):
    """doc/error_qs.MD:98-101 of the reference: beta(0.4, 0.1) seed 42."""
    o = oracle.lib()
    b = np.zeros(4)
    o.vgl_oracle_beta_std_draws(0.4, 0.1, 42, 4, b.ctypes.data)
    assert [f"{x:.6f}" for x in b] == ["0.621323", "0.960007", "0.525474", "0.002457"]


def test_host_program_qs_to_errprob_table():
    """QS_TO_ERRPROB (shared.h:493 over the literals of shared.cpp:31), as the host program restates it for the
    gl_error_prob lines of -printGlError: equal to the reference's table for every quality score."""
    import subprocess
    binp = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
    if not os.path.exists(binp):
        pytest.skip("vcfgl_hip not built")
    qs = list(range(0, 80))
    out = subprocess.run([binp, "--qs-to-errprob"] + [str(q) for q in qs], capture_output=True, text=True, check=True).stdout.split()
    assert _same(np.array([float(x) for x in out]), REF["qs_to_errprob"])
