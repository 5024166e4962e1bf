"""What the GL output tail must write, as exact functions of the GL that was written -- TEST INFRASTRUCTURE.

Reads neither the oracle nor the kernels: from a tile's GL (float32 bit patterns), n_alleles and site_status it states

  PL     the reference's `lroundf(-10.0 * gl)` capped at 255 (vcfgl.cpp:907-939), in exact rational arithmetic: the product
         Fraction(-10) * Fraction(gl), rounded to the nearest float32 (ties to even) because lroundf() takes a float argument, then
         rounded half away from zero; -inf -> 255; missing -> missing.
         The float32 step is not idle: gl = 14260633 * 2^-24 (0.85000002...) has -10 gl = 8.5 - 3 * 2^-23 exactly, which is
         8.5 as a float32 -- the reference writes 9 where rounding the exact product would give 8 (about one GL value in 10^5
         - 10^6 lies that close below a half-integer).  test_gl_tail_model_cpu.py pins that case against the C library's lroundf.
  pl_u8  PL capped at 255, 255 also standing for missing.
  GP     10^gl_i / sum_j 10^gl_j over the site's own genotype count (vcfgl.cpp:941-970), in mpmath at 200 bits, with the bound
         that float32 arithmetic in ANY order of summation keeps:

             |gp - exact| <= 18 * 2^-24 * exact + 2^-149

         one rounding per 10^x, at most NG - 1 = 14 for the sum, one for the division = 16 roundings in any value (18: those
         with a margin of two, which also takes the second-order terms); 2^-149 for terms that are float32 subnormals.  The
         sum is at least 1 because the largest GL of an evaluation is exactly 0.

Arrays are canonical planes [site][G][sample] (canon() brings a sample-major tile into that shape)."""
import math
from fractions import Fraction

import mpmath
import numpy as np

F32_MISSING_BITS = 0x7F800001
F32_NEG_INF_BITS = 0xFF800000
I32_MISSING = -(2 ** 31)
MAXPL = 255
SITE_OK = 0
GP_ROUNDINGS = 18
MP = mpmath.mp.clone()
MP.prec = 200


def mixed_sites(n_sites, n_samples, seed=100, missing=0.03):
    """true genotypes (the `gt` bytes of a tile) with one to four alleles per site in turn and missing calls, so that with few
    base-call errors every allele count occurs among the sites"""
    out = []
    for i in range(n_sites):
        rng = np.random.default_rng(seed + i)
        pool = rng.permutation(4)[: 1 + i % 4]
        al = pool[rng.integers(0, len(pool), size=(n_samples, 2))].astype(np.uint8)
        al = np.where(rng.random((n_samples, 2)) < missing, 0xF, al).astype(np.uint8)
        out.append(al[:, 0] | (al[:, 1] << 4))
    return np.stack(out).astype(np.uint8)


def n_genotypes(n_alleles):
    return n_alleles * (n_alleles + 1) // 2


def canon(tile, name, sample_major, fill):
    """a planeG field of a tile as [site][G][sample] (float32 fields as their uint32 bit patterns); what the layout does not hold
    for a site (genotypes beyond its own count in the sample-major layout) is set to `fill`"""
    a = tile.numpy(name)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    if not sample_major:
        return a.copy()
    S, G, N = a.shape
    out = np.full((S, G, N), fill, dtype=a.dtype)
    na = tile.numpy("n_alleles")
    st = tile.numpy("site_status")
    for s in range(S):
        ng = n_genotypes(int(na[s])) if st[s] >= 0 else 0          # a skipped site holds no values at all
        if ng:
            out[s, :ng, :] = a[s].reshape(-1)[: N * ng].reshape(N, ng).T      # the site's [sample][genotype] records
    return out


def canon_bits(tile, name, sample_major):
    """a float32 planeG field as uint32 bit patterns [site][G][sample], the missing pattern where the layout holds nothing"""
    return canon(tile, name, sample_major, F32_MISSING_BITS)


def round_to_float32(x):
    """the float32 nearest to the rational x >= 0 (ties to even), as a Fraction; +inf beyond the largest finite value"""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                                                      # 2^e <= x < 2^(e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)                          # the spacing of float32 at x (subnormals: 2^-149)
    n = x / q
    f = n.numerator // n.denominator
    r = n - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and (f & 1)):
        f += 1
    y = f * q
    return y if y < Fraction(2) ** 128 else None


def pl_of_bits(bits):
    """PL of one float32 GL bit pattern (see the module's docstring)"""
    bits = int(bits)
    if bits == F32_MISSING_BITS:
        return I32_MISSING
    if bits == F32_NEG_INF_BITS:
        return MAXPL
    gl = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
    assert not math.isnan(gl) and gl <= 0.0, hex(bits)
    x = round_to_float32(Fraction(-10) * Fraction(gl))
    if x is None or x > MAXPL:
        return MAXPL
    return int(math.floor(x + Fraction(1, 2)))                      # x >= 0: half away from zero is half up


def pl_exact(gl_bits):
    """int32 PL for an array of GL bit patterns"""
    gl_bits = np.asarray(gl_bits, dtype=np.uint32)
    u, inv = np.unique(gl_bits.reshape(-1), return_inverse=True)
    pl = np.array([pl_of_bits(b) for b in u], dtype=np.int64)
    return pl[inv].reshape(gl_bits.shape).astype(np.int32)


def pl_u8_exact(pl):
    return np.where(pl == I32_MISSING, 255, np.minimum(pl, 255)).astype(np.uint8)


def exp10_mp(gl):
    """10^gl for a float (exact conversion) at 200 bits; -inf -> 0"""
    if gl == -math.inf:
        return MP.mpf(0)
    return MP.power(10, MP.mpf(float(gl)))


def gp_exact(gls):
    """the exact GP of one evaluation: a list of mpf, one per GL"""
    p = [exp10_mp(g) for g in gls]
    s = MP.fsum(p)
    return [x / s for x in p]


def valid_mask(gl_bits, n_alleles, site_status):
    """[site][G][1]: the genotypes a written site has"""
    S, G, _ = gl_bits.shape
    ng = np.where(np.asarray(site_status) == SITE_OK, np.asarray(n_alleles) * (np.asarray(n_alleles) + 1) // 2, 0)
    return (np.arange(G)[None, :] < ng[:, None])[:, :, None]


def check_gl_invariants(gl_bits, n_alleles, site_status, fmt_dp):
    """every sample with reads: each GL <= 0 and the largest exactly 0; a sample without reads, a genotype beyond the site's count and
    a site that is not written carry the missing pattern.  Returns the mask [site][G][sample] of the values that exist."""
    gl_bits = np.asarray(gl_bits, dtype=np.uint32)
    live = valid_mask(gl_bits, n_alleles, site_status) & (np.asarray(fmt_dp) > 0)[:, None, :]
    assert np.all(gl_bits[~live] == F32_MISSING_BITS), "a value that does not exist is not the missing pattern"
    gl = gl_bits.view(np.float32)
    assert not np.any(gl_bits[live] == F32_MISSING_BITS) and not np.any(np.isnan(gl[live])), "a missing or NaN GL in an evaluation with reads"
    assert np.all(gl[live] <= 0.0), "GL > 0"
    top = np.where(live, gl, -np.inf).max(axis=1)                   # [site][sample]
    has = live.any(axis=1)
    assert np.all(top[has] == 0.0), "the largest GL of an evaluation is not 0"
    return live


def check_pl(gl_bits, pl, pl_u8=None):
    """PL (and the byte plane) equal to the exact function of GL, everywhere"""
    want = pl_exact(gl_bits)
    bad = np.argwhere(want != np.asarray(pl))
    assert bad.size == 0, f"PL differs from the exact value at {bad[:5].tolist()}: got {np.asarray(pl)[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    if pl_u8 is not None:
        assert np.array_equal(pl_u8_exact(want), np.asarray(pl_u8)), "pl_u8"
    return want


def check_gp(gl_bits, gp_bits, live, mp_budget=1500):
    """GP within gp_bound() of the exact value for EVERY value: a float64 evaluation (error < 1e-14 relative, against a bound of 1e-6)
    settles what lies below 0.99 of the bound, mpmath whatever does not -- and, whatever float64 says, up to `mp_budget` values of
    the evaluations that hold -inf, a 10^x below the float32 normal range, or come up on a fixed stride.
    Returns (values checked, values taken to mpmath, worst error / bound)."""
    gl_bits = np.asarray(gl_bits, dtype=np.uint32)
    gp_bits = np.asarray(gp_bits, dtype=np.uint32)
    assert np.all(gp_bits[~live] == F32_MISSING_BITS), "GP of a value that does not exist is not the missing pattern"
    with np.errstate(invalid="ignore"):                             # (the missing pattern is a signalling NaN)
        gl = gl_bits.view(np.float32).astype(np.float64)
        gp = gp_bits.view(np.float32).astype(np.float64)
    assert not np.any(np.isnan(gp[live])), "NaN (or the missing pattern) in the GP of an evaluation with reads"
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(live, np.power(10.0, np.where(live, gl, 0.0)), 0.0)
    tot = p.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        ex = np.where(live, p / np.where(tot > 0, tot, 1.0), 0.0)
    ratio = np.where(live, np.abs(gp - ex) / (GP_ROUNDINGS * 2.0 ** -24 * ex + 2.0 ** -149), 0.0)
    ev_live = live.any(axis=1)                                       # [site][sample]
    special = (live & ((gl_bits == F32_NEG_INF_BITS) | (gl < -37.9))).any(axis=1)
    todo = set(map(tuple, np.argwhere((ratio > 0.99).any(axis=1))))
    used = sum(int(live[s, :, n].sum()) for s, n in todo)
    order = [tuple(x) for x in np.argwhere(special)] + [tuple(x) for x in np.argwhere(ev_live)[::7]]
    for s, n in order:
        if (s, n) in todo:
            continue
        k = int(live[s, :, n].sum())
        if used + k > mp_budget:
            break
        todo.add((s, n))
        used += k
    worst_mp = 0.0
    for s, n in sorted(todo):
        g = np.flatnonzero(live[s, :, n])
        exact = gp_exact([float(gl_bits[s, i, n:n + 1].view(np.float32)[0]) for i in g])
        for i, e in zip(g, exact):
            got = MP.mpf(float(gp[s, i, n]))
            r = abs(got - e) / (GP_ROUNDINGS * MP.mpf(2) ** -24 * e + MP.mpf(2) ** -149)
            worst_mp = max(worst_mp, float(r))
            assert r <= 1, f"GP[{s}, {i}, {n}] = {gp[s, i, n]!r}: exact {float(e)!r}, error / bound {float(r):.3f}"
    rest = ratio.copy()
    for s, n in todo:
        rest[s, :, n] = 0.0
    assert not np.any(rest > 0.99)                                   # (everything above went to mpmath)
    return int(live.sum()), used, max(worst_mp, float(rest.max()) if rest.size else 0.0)


def gp_in_reference_order(gl_bits, live):
    """GP as float32 arithmetic in the reference's order gives it (vcfgl.cpp:948-968): each 10^gl rounded to float32, summed in float32
    from the first genotype to the last, divided in float32.  (10^gl through float64: the double rounding can move one float32 in about
    2^-28 -- this function serves a count of non-identical values, not a bound.)  uint32 bit patterns, missing where nothing exists."""
    with np.errstate(over="ignore", invalid="ignore"):
        gl = np.asarray(gl_bits, dtype=np.uint32).view(np.float32).astype(np.float64)
        p = np.where(live, np.power(10.0, np.where(live, gl, 0.0)), 0.0).astype(np.float32)
    tot = np.zeros((p.shape[0], p.shape[2]), dtype=np.float32)
    for i in range(p.shape[1]):
        tot = (tot + p[:, i, :]).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        gp = (p / tot[:, None, :]).astype(np.float32)
    return np.where(live, gp.view(np.uint32), np.uint32(F32_MISSING_BITS))


def float32_of_mp(x):
    """the float32 nearest to the non-negative mpf x (ties to even), rounded in ONE step from the 200-bit value: its bit pattern"""
    if x == 0:
        return 0
    m, e = MP.frexp(x)                                               # x = m 2^e, m in [1/2, 1)
    e = int(e) - 1                                                   # 2^e <= x < 2^(e + 1)
    sh = max(e, -126) - 23
    n = MP.ldexp(x, -sh)
    f = int(MP.floor(n))
    r = n - f
    if r > MP.mpf(0.5) or (r == MP.mpf(0.5) and (f & 1)):
        f += 1
    v = np.float32(math.ldexp(f, sh))                                # exact: f < 2^24 + 1, a float32 value by construction
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])
