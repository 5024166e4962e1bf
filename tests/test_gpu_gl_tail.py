"""The GL output tail -- PL, pl_u8, GP and the three helpers behind them (pl_of, exp10_nonpos, log10_unit: vgl_common.hip.h) -- against
references that owe nothing to the kernels or to the oracle.

1. Dumps (vgl_dbg_gl_tail, hooks build): each helper over a caller's array, compared with exact rational arithmetic (PL) and with
   mpmath at 200 bits (10^x, log10) -- the device's own pow / log10, which the sweeps of tests/test_gpu_bounds.py use over the whole
   domain, are implementations too, not the truth.
2. Tiles: tests/gl_tail_model.py applied to what every build with a tail of its own writes -- k_gl<4 | 5, 2>, k_gl<., 1>,
   --precise-gl 1, k_gl2 and k_gl_redo, the fused build -- in both output layouts, with pl_u8, at N = 1 / 63 / 65 / 130 (a partial
   wavefront, one lane over, two wavefronts and a ragged third) and 7 ... 33 sites.  Each case asserts from vgl_ctx_info() which build
   ran, and that what it is meant to produce (-inf, a PL of 255, readless samples, skipped sites, 10^GL in the float32 subnormal
   range) does occur."""
import ctypes as C
import math

import numpy as np
import pytest

import gl_tail_model as M
from gl_cases import TILE_CASES, case_ids, simulate_case              # (the case table: shared with test_gpu_gl_body.py)
from vcfgl_amd import _abi

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ dumps
def dump(fn, x):
    lib = _abi.load_library(hooks=True)
    lib.vgl_dbg_gl_tail.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    x = np.ascontiguousarray(x)
    out = np.zeros(x.shape, dtype=np.uint32 if fn == 2 else np.float64)
    assert lib.vgl_dbg_gl_tail(fn, x.ctypes.data, out.ctypes.data, x.size) == 0
    return out


def f32bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_pl_of_equals_exact_rational_rounding():
    """pl_of over 6e4 GLs against gl_tail_model.pl_exact (Fractions): -0x1.999998p-5 -> 0 (the one float where trunc(x + 0.5f) is
    wrong) and its neighbours -> 0 / 1; five floats around every k + 0.5 / -10, k = 0 .. 255; 14260633 x 2^-24 (exact product below 8.5,
    float32 product 8.5: the reference's lroundf gives 9); +-0; the cap at 25.45 / 25.5; -3e38; -inf; random GLs down to -30"""
    g0 = int(f32bits(float.fromhex("-0x1.999998p-5")))
    named = np.array([g0 - 1, g0, g0 + 1, 0x00000000, 0x80000000, M.F32_NEG_INF_BITS, int(f32bits(-3e38)), int(f32bits(-14260633 * 2.0 ** -24))], dtype=np.uint32)
    assert M.pl_exact(named).tolist() == [0, 0, 1, 0, 0, 255, 255, 9]
    half = f32bits(-(np.arange(256) + 0.5) / 10.0).astype(np.int64)
    near = (half[:, None] + np.arange(-2, 3)[None, :]).reshape(-1).astype(np.uint32)
    rng = np.random.default_rng(11)
    rand = f32bits(-(10.0 ** rng.uniform(-6, math.log10(30.0), 58000)))
    bits = np.concatenate([named, near, rand])
    assert bits.size <= 100_000
    got = dump(2, bits.view(np.float32))
    want = M.pl_exact(np.where(bits == 0, 0x80000000, bits)).astype(np.int64)      # (+0: the model takes GL <= 0; PL 0 either way)
    bad = np.flatnonzero(got.astype(np.int64) != want)
    print(f"pl_of: {bits.size} arguments, {bad.size} differ from the exact value")
    assert got[:3].tolist() == [0, 0, 1]
    assert bad.size == 0, [(hex(int(bits[i])), int(got[i]), int(want[i])) for i in bad[:5]]


def exp10_args():
    rng = np.random.default_rng(12)
    f = np.float32
    x0, x1, x2 = math.log10(2.0) * -150, math.log10(2.0) * -149, math.log10(2.0) * -126      # zero / smallest subnormal / smallest normal float32
    def around(x, k=40):
        b = int(f32bits(x))
        return np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32).view(f)
    parts = [np.array([-0.0, -2.0 ** -149, -1e-30, -1e-8, -1.0, -2.0, -37.9, -45.2, -300.0, -307.9, -329.9, -330.0, -331.0, -3e38, -np.inf], dtype=f),
             around(x0), around(x1), around(x2), around(-38.0), around(-300.0), around(-1.0), around(-0.30103),
             rng.uniform(-45.2, -37.9, 6000).astype(f), rng.uniform(-46.0, 0.0, 20000).astype(f), rng.uniform(-300.0, -46.0, 6000).astype(f),
             (-(10.0 ** rng.uniform(-12, 0, 6000))).astype(f), (-np.arange(0, 400) * 0.1).astype(f),
             np.array([0xBF016221], dtype=np.uint32).view(f)]       # (where the sweep of tests/test_gpu_bounds.py found the largest distance from the device's pow)
    return np.concatenate(parts)


def exp10_edge_args(sign, n=2500):
    """float32 x in [-40, 0) whose reduced argument f = x log2(10) - rint(x log2(10)) lies within 0.05 of sign / 2: the ends of the
    polynomial's range, where a missing high-order term shows"""
    rng = np.random.default_rng(14)
    x = rng.uniform(-40.0, 0.0, 40 * n).astype(np.float32)
    y = x.astype(np.float64) * 3.3219280948873622
    f = y - np.rint(y)
    x = x[(f * sign >= 0.45)]
    assert x.size >= n
    return x[:n]


def test_exp10_nonpos_against_mpmath():
    """exp10_nonpos over 4e4 float32 arguments (what the kernels pass: (double)acc[i]) against 10^x at 200 bits: the double result within
    1e-15 relative for x >= -300 (the CPU restatement of its steps measured 1.7e-16, a pencil bound on its roundings
    gives 2.1e-16); its float32 never more than one unit in the last place from the correctly rounded float32 of the exact value
    (rounded in one step from the 200-bit value), subnormal results included, at most a share of 1e-5 of the finite nonzero ones not
    identical, and zero wherever the correctly rounded float32 is zero.  Arguments: -0, the float32 neighbourhoods of log10 2^-150 /
    2^-149 / 2^-126 (zero | subnormal | normal results), -37.9 ... -45.2 densely, [-300, 0], tiny |x|, -330 and beyond, -inf."""
    x = exp10_args()
    assert x.size <= 100_000 and np.all(x <= 0)
    got = dump(1, x.astype(np.float64))
    worst, worst_x, nonid, nz, far = 0.0, 0.0, 0, 0, []
    for xi, gi in zip(x.tolist(), got.tolist()):
        ex = M.exp10_mp(xi)
        if xi >= -300.0:
            r = float(abs(M.MP.mpf(gi) - ex) / ex)
            if r > worst:
                worst, worst_x = r, xi
        want = M.float32_of_mp(ex)
        have = int(f32bits(gi))                                     # (the double's own rounding to float32, as the kernels' cast)
        if want != 0:
            nz += 1
            nonid += have != want
        if abs(have - want) > 1 or (want == 0 and have != 0):
            far.append((xi, have, want))
    print(f"exp10_nonpos: {x.size} arguments, worst relative error of the double result {worst:.3e} at x = {worst_x!r} ({float(worst_x).hex()}); "
          f"{nonid} of {nz} finite nonzero float32 results not the correctly rounded one")
    assert not far, far[:5]
    assert worst <= 1e-15
    assert nonid <= 1e-5 * nz
    # The mean SIGNED relative error at the ends of the reduced range (|f| >= 0.45, t = f ln 2 up to 0.3466), by sign of f.  What is
    # systematic there by construction: the Taylor remainder t^14 / 14! <= 4.2e-18, the constant 0.69314718055994531 (2.32e-17 below
    # ln 2: f x 2.32e-17 <= 1.2e-17 in t) and the rounded coefficients (< 1e-18) -- 1.7e-17 in all; the roundings themselves average out
    # (each below 1.2e-16, 2500 arguments: 2.4e-18 standard deviation of the mean).  Three times the systematic part is allowed; a
    # polynomial one term short carries t^13 / 13! = 1.7e-16 there.
    for sign in (1, -1):
        xe = exp10_edge_args(sign)
        ge = dump(1, xe.astype(np.float64))
        mean = float(sum((M.MP.mpf(g) - M.exp10_mp(xv)) / M.exp10_mp(xv) for xv, g in zip(xe.tolist(), ge.tolist())) / xe.size)
        print(f"exp10_nonpos: mean signed relative error over {xe.size} arguments with f {'>= 0.45' if sign > 0 else '<= -0.45'}: {mean:.3e}")
        assert abs(mean) <= 5e-17


def log10_args():
    rng = np.random.default_rng(13)
    r2 = 0.70710678118654752
    mant = 1.0 + rng.integers(0, 1 << 52, 12000).astype(np.float64) * 2.0 ** -52
    e = np.concatenate([10.0 ** rng.uniform(-16, math.log10(0.75), 5000), 10.0 ** rng.uniform(-7, math.log10(0.75), 3000), [1e-16, 1e-7, 0.75, 0.5, 2.0 ** -53]])
    sw = np.nextafter(r2, 0) + (rng.integers(-4096, 4097, 3000) * 2.0 ** -53)
    parts = [np.array([1.0, 0.0, 5e-324, 2.2250738585072014e-308, float.fromhex("0x1.6927bc0fb3561p-1"), r2, np.nextafter(r2, 0), np.nextafter(r2, 1), 0.5, 0.25]),
             np.ldexp(mant, -1 - rng.integers(0, 1022, mant.size)), np.ldexp(mant[:2000], -1 - rng.integers(1022, 1074, 2000)),
             1.0 - np.arange(0, 3000) * 2.0 ** -53, np.ldexp(sw, -rng.integers(0, 1022, sw.size)), sw,
             1.0 - e, (1.0 - e) / 2.0 + (e / 3.0) * 0.5, e / 3.0]
    x = np.concatenate(parts)
    return x[(x >= 0.0) & (x <= 1.0)]


def test_log10_unit_against_mpmath():
    """log10_unit over 4e4 doubles of [0, 1] against log10 at 200 bits, relative error <= 1e-15 (the CPU restatement of its steps
    measured 4.6e-16 at 0x1.6927bc0fb3561p-1, just below sqrt(1/2), where e ln 2 and ln m cancel most -- that argument is in the set):
    random mantissas at every exponent down to the subnormals, 1 - k 2^-53, both sides of the sqrt(1/2) switch at every exponent,
    and the read loop's three arguments 1 - e, (1 - e) / 2 + e / 6, e / 3 for e from 0.75 down to 1e-16; exactly 0 at 1, -inf at 0"""
    x = log10_args()
    assert x.size <= 100_000
    got = dump(0, x)
    assert x[0] == 1.0 and got[0] == 0.0 and not np.signbit(got[0]) and x[1] == 0.0 and got[1] == -np.inf
    worst, worst_x = 0.0, 1.0
    for xi, gi in zip(x.tolist(), got.tolist()):
        if xi in (0.0, 1.0):
            assert gi == (0.0 if xi == 1.0 else -math.inf)
            continue
        ex = M.MP.log10(M.MP.mpf(xi))
        r = float(abs((M.MP.mpf(gi) - ex) / ex))
        if r > worst:
            worst, worst_x = r, xi
    print(f"log10_unit: {x.size} arguments, worst relative error {worst:.3e} at x = {float(worst_x).hex()}")
    assert worst <= 1e-15


# ------------------------------------------------------------------------------------------------ tiles
@pytest.mark.parametrize("name,sm,N", TILE_CASES, ids=case_ids(TILE_CASES))
def test_tile_tags_are_exact_functions_of_the_gl_written(name, sm, N, monkeypatch):
    """every PL and pl_u8 equals the exact rounding of -10 GL, every GP lies within 18 x 2^-24 exact + 2^-149 of the exact
    10^gl_i / sum 10^gl_j (mpmath for the -inf / subnormal evaluations, a stride of the rest and whatever float64 cannot settle), GL
    obeys its invariants (<= 0, largest exactly 0, missing where nothing exists); and GP is float32 arithmetic in the reference's
    order -- first genotype to last -- for all but a share of 1e-5 of the values (an order of summation is within the bound whichever
    it is; only this count tells them apart).  What the case is meant to produce is asserted (PATHS)."""
    t, occur = simulate_case(name, sm, N, monkeypatch)
    na, st, dp = t.numpy("n_alleles"), t.numpy("site_status"), t.numpy("fmt_dp")
    gl = M.canon_bits(t, "gl", sm)
    live = M.check_gl_invariants(gl, na, st, dp)
    want = M.check_pl(gl, M.canon(t, "pl", sm, M.I32_MISSING), M.canon(t, "pl_u8", sm, 255))
    glf = gl.view(np.float32)
    n_inf, n_sub = int((gl[live] == M.F32_NEG_INF_BITS).sum()), int(((glf[live] < -37.93) & (glf[live] > -45.15)).sum())
    n_cap, n_skip, n_dp0 = int((want[live] == 255).sum()), int((st < 0).sum()), int(((dp == 0) & (st == 0)[:, None]).sum())
    msg = f"{name} {'sample-major' if sm else 'planes'} N={N}: {int(live.sum())} values, n_alleles {sorted(set(na[st == 0].tolist()))}, -inf {n_inf}, 10^GL subnormal {n_sub}, PL 255 {n_cap}, skipped sites {n_skip}, readless samples {n_dp0}"
    if not occur.get("no_gp"):
        gp = M.canon_bits(t, "gp", sm)
        n, n_mp, worst = M.check_gp(gl, gp, live, mp_budget=600)
        nonid = int((M.gp_in_reference_order(gl, live) != gp).sum())
        msg += f"; GP: {n_mp} values against mpmath, worst error / bound {worst:.3f}, {nonid} not identical to the float32 arithmetic in genotype order"
        assert nonid <= max(1, math.ceil(1e-5 * n)), msg
    print(msg)
    assert live.sum() > 0
    if "alleles" in occur:
        need = occur["alleles"] if N >= 63 else set(sorted(occur["alleles"])[:2])
        assert set(na[st == 0].tolist()) >= need, msg
    if occur.get("inf"):
        assert n_inf > 0 and n_cap >= n_inf, msg
    if occur.get("cap") and N >= 63:
        assert n_cap > 0, msg
    if occur.get("sub") and N >= 63:
        assert n_sub > 0 and float(glf[live][np.isfinite(glf[live])].min()) < -45.2, msg
    if occur.get("skip"):
        assert (n_skip > 0) == (N <= 5) and n_dp0 + n_skip > 0, msg
        if N > 5:
            assert n_dp0 > 0, msg
    if name != "rm-empty-sites" and N >= 63:
        assert ((dp == 0) & (st == 0)[:, None]).any(), msg           # 3 % missing calls: samples without reads at written sites
