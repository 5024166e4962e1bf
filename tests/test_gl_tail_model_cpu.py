"""tests/gl_tail_model.py against the oracle's binary output (no GPU): the PL, pl_u8 and GP the oracle writes -- which the reference's
goldens pin (tests/test_oracle_golden.py, test_oracle_vs_ref.py) -- must satisfy the exact model, and the GL it writes the model's
invariants.  That validates the model; tests/test_gpu_gl_tail.py then holds the device tiles to it."""
import ctypes as C
import ctypes.util
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import gl_tail_model as M
from vcfgl_amd import VcfglArgs, _abi


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


CASES = {
    # -doUnobserved 1: 2 ... 5 alleles per site, missing calls, samples without reads
    "unobserved1": (dict(seed=5, depth=2.5, error_rate=0.002, do_unobserved=1), 37, 21, False),
    # -doUnobserved 5: every site has 5 alleles / 15 genotypes; sample-major records
    "unobserved5-sample-major": (dict(seed=6, depth=9.0, error_rate=0.02, do_unobserved=5), 65, 9, True),
    # --error-rate 0 with --precise-gl 1: a read's homF term is log10(0) = -inf, so -inf stands next to 0 and PL is 255 there
    # (without --precise-gl 1 the score is capped at 63 and every term is finite: the next case)
    "error-rate-0-precise": (dict(seed=7, depth=4.0, error_rate=0.0, do_unobserved=1, precise_gl=1), 40, 17, False),
    # --error-rate 0, score 63: 6.3 per mismatching read -- GL passes -37.9 ... -45.2, where 10^x is a float32 subnormal, and goes on to zero
    "error-rate-0-score-63": (dict(seed=7, depth=4.0, error_rate=0.0, do_unobserved=1), 40, 17, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_tags_satisfy_the_exact_model(oracle, name):
    kw, N, S, sm = CASES[name]
    args = VcfglArgs(add_pl=1, add_gp=1, **kw)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    if sm:
        args.out_layout = _abi.VGL_LAYOUT_SAMPLE_MAJOR
    gt = M.mixed_sites(S, N)
    t = oracle.Oracle(args, N).simulate(0, gt, fields=["fmt_dp", "gl", "pl", "gp", "pl_u8"])
    gl = M.canon_bits(t, "gl", sm)
    live = M.check_gl_invariants(gl, t.numpy("n_alleles"), t.numpy("site_status"), t.numpy("fmt_dp"))
    want = M.check_pl(gl, M.canon(t, "pl", sm, M.I32_MISSING), M.canon(t, "pl_u8", sm, 255))
    gp = M.canon_bits(t, "gp", sm)
    n, n_mp, worst = M.check_gp(gl, gp, live)
    glf = gl.view(np.float32)
    n_inf, n_sub = int((gl[live] == M.F32_NEG_INF_BITS).sum()), int(((glf[live] < -37.93) & (glf[live] > -45.15)).sum())
    print(f"{name}: {n} values, {n_mp} of them against mpmath, worst GP error / bound {worst:.3f}; n_alleles {sorted(set(t.numpy('n_alleles').tolist()))}, "
          f"-inf {n_inf}, 10^GL subnormal {n_sub}, PL 255 {int((want[live] == 255).sum())}, readless samples {int((t.numpy('fmt_dp') == 0).sum())}")
    assert n > 1000 and n_mp > 100 and (t.numpy("fmt_dp") == 0).any()
    nonid = int((M.gp_in_reference_order(gl, live) != gp).sum())
    assert nonid <= max(1, math.ceil(1e-5 * n)), f"{nonid} of {n} GP values are not the float32 arithmetic of the reference's order"
    if name == "unobserved1":
        assert set(t.numpy("n_alleles").tolist()) >= {2, 3, 4, 5}
    if name == "unobserved5-sample-major":
        assert (t.numpy("n_alleles") == 5).all()
    if name == "error-rate-0-precise":
        assert n_inf > 0 and (want[live] == 255).any()
    if name == "error-rate-0-score-63":
        assert n_sub > 0 and (want[live] == 255).any()


def test_pl_model_named_values():
    """the value that needs pl_of's compare (gl = -0x1.999998p-5: -10 gl = 0.5 - 2^-25, PL 0) and its neighbours; the cap; -inf; -0;
    missing; and a GL whose exact product lies below a half-integer but whose float32 product is the half-integer -- the C library's
    lroundf on the float argument, as the reference calls it (vcfgl.cpp:931), agrees with the model on all of them"""
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.lroundf.argtypes, libm.lroundf.restype = [C.c_float], C.c_long
    g0 = float.fromhex("-0x1.999998p-5")
    named = {bits_of(g0): 0, bits_of(g0) - 1: 0, bits_of(g0) + 1: 1, bits_of(-0.0): 0, bits_of(-25.45): 255, bits_of(-25.5): 255,
             bits_of(-3e38): 255, M.F32_NEG_INF_BITS: 255, M.F32_MISSING_BITS: M.I32_MISSING,
             bits_of(-14260633 * 2.0 ** -24): 9}
    for b, want in named.items():
        assert M.pl_of_bits(b) == want, (hex(b), M.pl_of_bits(b), want)
    assert Fraction(-10) * Fraction(-14260633, 2 ** 24) == Fraction(17, 2) - Fraction(3, 2 ** 23)      # exactly: below 8.5
    rng = np.random.default_rng(1)
    some = np.concatenate([rng.integers(0x80000000, 0xC3800000, 4000, dtype=np.uint64).astype(np.uint32),
                           np.array([b for b in named if b not in (M.F32_NEG_INF_BITS, M.F32_MISSING_BITS)], dtype=np.uint32)])
    for b in some:
        gl = float(np.array([b], dtype=np.uint32).view(np.float32)[0])
        if -10.0 * gl < 2.0 ** 31:                                  # (beyond: lroundf's result is unspecified; GL never gets there)
            assert M.pl_of_bits(b) == min(libm.lroundf(-10.0 * gl), 255), hex(int(b))
    assert M.pl_u8_exact(np.array([0, 254, 255, M.I32_MISSING], dtype=np.int32)).tolist() == [0, 254, 255, 255]


def test_float32_rounding_of_exact_values():
    """round_to_float32 / float32_of_mp: ties to even, subnormals, and agreement with numpy on doubles"""
    assert M.round_to_float32(Fraction(1) + Fraction(1, 2 ** 24)) == 1                       # tie -> even
    assert M.round_to_float32(Fraction(1) + Fraction(3, 2 ** 24)) == Fraction(1) + Fraction(1, 2 ** 22)
    assert M.round_to_float32(Fraction(3, 2 ** 150)) == Fraction(1, 2 ** 148)                # subnormal tie -> even
    assert M.round_to_float32(Fraction(1, 2 ** 150)) == 0
    rng = np.random.default_rng(2)
    for x in np.concatenate([10.0 ** rng.uniform(-46, 0, 500), [2.0 ** -149, 2.0 ** -150 * 1.0000001, 1.0, 2.0 ** -126]]):
        want = int(np.array([x], dtype=np.float64).astype(np.float32).view(np.uint32)[0])
        assert M.float32_of_mp(M.MP.mpf(float(x))) == want, x
        assert M.round_to_float32(Fraction(float(x))) == Fraction(float(np.float32(x))), x
    assert M.float32_of_mp(M.MP.mpf(2) ** -150) == 0 and M.float32_of_mp(M.MP.mpf(2) ** -150 + M.MP.mpf(2) ** -190) == 1
