"""The body of the GL kernels and the tags that are sums over the reads, stated from the reads a tile drew -- TEST INFRASTRUCTURE.

Imports nothing from the library or the oracle.  From the dumps of a tile call (`reads`: (score << 2) | base per read, `read_errp`:
the per-read error probability of --error-qs 2) and fmt_dp, alleles2acgt, n_alleles, site_status it states

  gl2_exact   GL model 2 from its definition, in float64.  For a read whose base is allele `ao`, with error probability e, the term of
              genotype (a1, a2) is

                  log10(1 - e)              a1 = a2 = ao
                  log10((1 - e) / 2 + e / 6)  exactly one of them is ao
                  log10(e / 3)              neither

              e = 10^(-q / 10) of the score q used for GL (table builds), or the read's own probability (--precise-gl 1; e = 0 gives
              0, log10 1/2 and -inf).  GL = the sum over the evaluation's reads minus its maximum, over ALL n_alleles of the site --
              the unobserved allele included, to which no read maps.
  gl2_replay  the reference's float32 recurrence in the dump's read order (gl_methods.cpp): per read every genotype's value becomes
              float32((double)value + term), then the float32 maximum is subtracted from every value in float32.  Terms: the
              seven-significant-digit table regenerated here (scores 0 .. 63), or log10 of e for --precise-gl 1 with the reference's
              literals (-0.30103 per read, -0.3010299956639812 for the fixed score).
  gl1_costs   GL model 1 ("revised MAQ", Li 2011) from its definition in exact rational arithmetic.
  counts_from_reads   DP, AD, INFO/DP, INFO/AD, I16 fields 1-12 and QS (exact rationals).

THE BOUND of gl2_exact on what float32 arithmetic in the reference's order can write.  Write S_g(k) for the exact sum of genotype g's
terms over reads 1 .. k, x_g(k) = S_g(k) - max_h S_h(k) for the exactly normalised value, v_g(k) for the float32 value after read k, and
u = 2^-24 (1 + 2^-20) (a float32 rounding; the margin takes the double rounding of the float64 sum, 2^-53, this model's own float64
roundings and every second-order product).  All values and terms are <= 0, so are their sums.

  One step.  a_g = fl(v_g(k-1) + t~_g) = v_g(k-1) + t_g + tau_g + d1_g, with t~ the term the kernel holds, tau_g = t~_g - t_g its
  literal error, |d1_g| <= u |v_g(k-1) + t~_g|.  m = max_g a_g = a_g' (comparisons are exact).  v_g(k) = fl(a_g - m) = a_g - m + d2_g,
  |d2_g| <= u |a_g - m|; v_g'(k) = 0 exactly.
  Own errors.  With C(k) = the sum of the maxima subtracted so far, v_g(k) = S_g(k) - C(k) + eps_g(k) where
  eps_g(k) = eps_g(k-1) + tau_g + d1_g + d2_g holds only roundings that touched g itself: subtracting the common m moves nothing
  between genotypes.  E_g(k) >= |eps_g(k)| is carried per genotype; E1_g = E_g(k-1) + |tau_g| + u P_g bounds it after the addition.
  Where the maximum's error goes.  v_g(k) = 0 at g = g', so C(k) = S_g'(k) + eps1_g' and
      a_g - m - x_g(k) = (S_h* - S_g') + eps1_g - eps1_g',   h* the exact maximum.
  g' beat h* in float32: S_g' + eps1_g' >= S_h* + eps1_h*, so 0 <= S_h* - S_g' <= eps1_g' - eps1_h*, and
      -(E1_g + E1_g') <= a_g - m - x_g(k) <= E1_g + E1_h*.
  g' is not known to the model, but x_g'(k) >= -(E1_g' + E1_h*) by the same inequality: the CANDIDATES are the genotypes with
  x_h(k) >= -(E1_h + E1_h*) (h* among them), and Etop1 = max of E1 over them.  This is the step at which the accumulated error of
  the genotype that becomes the maximum is carried to every other value:
      |v_g(k) - x_g(k)| <= B_g(k) = E1_g + Etop1 + u Q_g,    Q_g = |x_g(k)| + E1_g + Etop1 >= |a_g - m|,
      E_g(k) = E1_g + u Q_g,
      P_g = |x_g(k-1) + t_g| + B_g(k-1) + |tau_g| >= |v_g(k-1) + t~_g|    (the magnitudes the roundings scale with, from the exact model).
  So three roundings per read reach a value -- its own addition, the addition on the maximum (inside Etop1), the subtraction -- each
  u times a magnitude known here; B_g(n) is the bound.  -inf stays -inf under all of this and must stand exactly where x_g is -inf.
  tau.  Table builds: half a unit of the seventh significant digit of the term, 0.5 x 10^(floor(log10 |t|) - 6); it enters E1_g for
  the value and, through Etop1, once more for the maximum.  --precise-gl 1: 2^-49 |t| + 2^-52 (log10 in double, and 1 - e rounded
  before it), and |-0.30103 - log10(1/2)| = 4.4e-9 on the one-match term of a per-read e = 0."""
import math
from fractions import Fraction

import mpmath
import numpy as np

F32_MISSING_BITS = 0x7F800001
SITE_OK = 0
CAP_BASEQ = 63
U = 2.0 ** -24 * (1.0 + 2.0 ** -20)
HET0_PER_READ = -0.30103                      # the reference's literal for log10(1/2) in the per-read path of --precise-gl 1
HET0_FIXED = -0.3010299956639812              # ... and in the fixed-score path
A1 = np.array([a1 for a2 in range(5) for a1 in range(a2 + 1)])     # genotype index a2 (a2 + 1) / 2 + a1, a1 <= a2 (VCF order)
A2 = np.array([a2 for a2 in range(5) for a1 in range(a2 + 1)])
MUTANTS = ("het_e3", "row_plus_1", "unobserved_as_0", "max_observed_only", "swap_hom")
_MP = mpmath.mp.clone()
_MP.prec = 200


# ------------------------------------------------------------------------------------------------ scores and terms
def exact_terms_mp(q):
    """the three terms of score q at 200 bits: (two match, one matches, none); log10(0) = -inf"""
    p = _MP.power(10, _MP.mpf(-q) / 10)
    lg = lambda v: _MP.mpf("-inf") if v == 0 else _MP.log10(v)
    return lg(1 - p), lg((1 - p) / 2 + p / 6), lg(p / 3)


def round7_mp(v):
    """an mpf rounded to seven significant digits (what the reference's table literals hold), as a float"""
    if v == 0 or _MP.isinf(v):
        return float(v)
    return float(_MP.nstr(v, 7, strip_zeros=False, min_fixed=-_MP.inf, max_fixed=_MP.inf))


_TABLE = {}


def table(qmax=CAP_BASEQ):
    """float64 [3][qmax + 1]: the regenerated score table, rows (two match, one matches, none)"""
    if qmax not in _TABLE:
        _TABLE[qmax] = np.array([[round7_mp(t) for t in exact_terms_mp(q)] for q in range(qmax + 1)]).T.copy()
    return _TABLE[qmax]


def score_of_errp(ep, flags, adjusted):
    """the (adjusted) quality score of an error probability (vcfgl.cpp:500-523): int(-10 log10 ep [+ adjust_by]), then the --qs-bins
    value or the cap at 63; arrays in, int64 out (-1: no score)"""
    ep = np.asarray(ep, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tmp = -10.0 * np.log10(ep)
        q = np.where((ep > 0) & (ep < 1), np.trunc(tmp + (flags.get("adjust_by", 0.499) if adjusted else 0.0)), -1.0)
    q = np.where(np.isnan(q), -1.0, q).astype(np.int64)
    if not adjusted or flags.get("fixed"):
        q = np.where(ep == 0.0, CAP_BASEQ, np.where(ep == 1.0, 0, q))
    bins = flags.get("qs_bins")
    if bins:
        out = np.full(q.shape, -1, dtype=np.int64)
        for lo, hi, val in reversed(list(bins)):                     # (the first matching bin wins)
            out = np.where((q >= lo) & (q <= hi), val, out)
        return out
    return np.minimum(q, CAP_BASEQ)


def gl_scores(reads, read_errp, flags):
    """the score every read enters GL with, [read][site][sample].  `reads` carries the RAW score (after --qs-bins), for every
    --adjust-qs (include/vcfgl_hip.h: the caller derives the adjusted score from the deviates as vcfgl.cpp:500-523 does); with
    --adjust-qs bit 1 GL takes the adjusted score, derived here from read_errp (--error-qs 2) or from --error-rate (fixed score)."""
    raw = np.asarray(reads).astype(np.int64) >> 2
    if not (flags.get("adjust_qs", 0) & 1):
        return raw
    if flags.get("error_qs", 0) == 2:
        return score_of_errp(read_errp, flags, True)
    return np.broadcast_to(score_of_errp(flags["error_rate"], dict(flags, fixed=1), True), raw.shape)


def _terms(q, e, flags, mutant, per_read):
    """(T, H, F, tauT, tauH, tauF, T~, H~, F~): exact terms, their literal error bounds and the terms the float32 recurrence adds"""
    with np.errstate(divide="ignore"):
        if not flags.get("precise_gl"):
            qq = q + 1 if mutant == "row_plus_1" else q
            e = np.power(10.0, -qq / 10.0)
            T, F = np.log10(1.0 - e), np.log10(e / 3.0)
            H = np.log10((1.0 - e) / 2.0 + e / (3.0 if mutant == "het_e3" else 6.0))
            tab = table(CAP_BASEQ + 1)
            tt = tuple(tab[i][qq] for i in range(3))
            tau = tuple(np.where(np.isfinite(t) & (t != 0), 0.5 * 10.0 ** (np.floor(np.log10(np.abs(np.where(np.isfinite(t) & (t != 0), t, 1.0)))) - 6.0), 0.0) for t in (T, H, F))
        else:
            z = e == 0.0
            T = np.where(z, 0.0, np.log10(1.0 - e))
            H = np.log10((1.0 - e) / 2.0 + e / (3.0 if mutant == "het_e3" else 6.0))
            F = np.log10(e / 3.0)
            if per_read:
                tt = (T, np.where(z, HET0_PER_READ, H), F)
            else:
                tt = (T, np.where(z, HET0_FIXED, H), np.where(z, -np.inf, np.log10(np.where(z, 1.0, e)) - 0.47712125471966244))
            tau = tuple(np.where(np.isfinite(t), 2.0 ** -49 * np.abs(np.where(np.isfinite(t), t, 0.0)) + 2.0 ** -52, 0.0) for t in (T, H, F))
            tau = (tau[0], tau[1] + np.where(z & per_read, abs(HET0_PER_READ - math.log10(0.5)), 0.0), tau[2])
    if mutant == "swap_hom":
        T, F, tau, tt = F, T, (tau[2], tau[1], tau[0]), (tt[2], tt[1], tt[0])
    return (T, H, F) + tau + tt


class Tile:
    """what the model reads of a tile: numpy arrays (canonical shapes) and the flags that decide which e a read has"""

    def __init__(self, reads, read_errp, fmt_dp, alleles2acgt, n_alleles, site_status, flags):
        self.reads, self.read_errp, self.fmt_dp = np.asarray(reads), (None if read_errp is None else np.asarray(read_errp)), np.asarray(fmt_dp)
        self.alleles2acgt, self.n_alleles, self.site_status, self.flags = np.asarray(alleles2acgt), np.asarray(n_alleles), np.asarray(site_status), dict(flags)
        S, N = self.fmt_dp.shape
        ok = self.site_status == SITE_OK
        self.depth = np.where(ok[:, None], self.fmt_dp, 0)           # reads that enter an evaluation
        assert self.reads.shape[1:] == (S, N) and self.reads.shape[0] >= self.depth.max(initial=0), "the dump is shorter than the tile's largest depth"
        self.nG = np.where(ok, self.n_alleles * (self.n_alleles + 1) // 2, 0)
        self.G = 15 if self.flags.get("do_unobserved", 1) in (1, 2, 4, 5) else 10
        self.acgt2allele = np.full((S, 4), -1, dtype=np.int64)
        self.unobs = np.full(S, -1, dtype=np.int64)                  # the allele index of <*> / <NON_REF>, -1: none
        for s in range(S):
            for a in range(int(self.n_alleles[s]) if ok[s] else 0):
                b = int(self.alleles2acgt[s, a])
                if 0 <= b < 4:
                    self.acgt2allele[s, b] = a
                elif b == 4:
                    self.unobs[s] = a
        self.live = (np.arange(self.G)[None, :, None] < self.nG[:, None, None]) & (self.depth > 0)[:, None, :]
        self.per_read = self.flags.get("error_qs", 0) == 2

    def read(self, r):
        """(active [S][N], allele of the read's base [S][N], score for GL, error probability) of read r"""
        act = r < self.depth
        base = self.reads[r].astype(np.int64) & 3
        ao = np.take_along_axis(self.acgt2allele, base, axis=1)
        assert np.all(ao[act] >= 0), "a read's base is not an allele of its site"
        errp = self.read_errp[r] if (self.per_read and self.read_errp is not None) else None
        q = gl_scores(self.reads[r], errp, self.flags)
        assert np.all((q[act] >= 0) & (q[act] <= CAP_BASEQ))
        if self.flags.get("precise_gl"):
            e = np.where(act, errp, 0.5) if self.per_read else np.full(act.shape, float(self.flags["error_rate"]))
        else:
            e = None
        return act, np.where(act, ao, 0), np.where(act, q, 0), e

    def matches(self, ao, mutant=None):
        """[S][G][N]: how many of a genotype's two alleles are the read's"""
        a1 = np.broadcast_to(A1[None, : self.G, None], (ao.shape[0], self.G, 1))
        a2 = np.broadcast_to(A2[None, : self.G, None], (ao.shape[0], self.G, 1))
        if mutant == "unobserved_as_0":
            un = self.unobs[:, None, None]
            a1, a2 = np.where(a1 == un, 0, a1), np.where(a2 == un, 0, a2)
        return (a1 == ao[:, None, :]).astype(np.int64) + (a2 == ao[:, None, :])


def _pick(k, t0, t1, t2):
    return np.where(k == 2, t2[:, None, :], np.where(k == 1, t1[:, None, :], t0[:, None, :]))


# ------------------------------------------------------------------------------------------------ GL model 2
def gl2_exact(tile, mutant=None):
    """(x, B, M): [site][G][sample] float64 -- the GL of the definition (nan where no value exists, -inf where the definition puts
    it), the bound on |float32 GL - x| derived in the module's docstring, and M_g = the largest finite |running normalised value| +
    |term| of the genotype.  `mutant`: one of MUTANTS, a deliberately wrong model (the power test)."""
    S, N = tile.depth.shape
    G = tile.G
    valid = np.broadcast_to((np.arange(G)[None, :, None] < tile.nG[:, None, None]), (S, G, N))
    top_ok = valid
    if mutant == "max_observed_only":
        un = tile.unobs[:, None, None]
        top_ok = valid & (A1[None, :G, None] != un) & (A2[None, :G, None] != un)
    x = np.zeros((S, G, N))
    E, B, M = np.zeros((S, G, N)), np.zeros((S, G, N)), np.zeros((S, G, N))
    fin0 = lambda a: np.where(np.isfinite(a), a, 0.0)
    with np.errstate(invalid="ignore"):
        for r in range(int(tile.depth.max(initial=0))):
            act, ao, q, e = tile.read(r)
            T, H, F, tT, tH, tF = _terms(q, e, tile.flags, mutant, tile.per_read)[:6]
            k = tile.matches(ao, mutant)
            t, tau = _pick(k, F, H, T), _pick(k, tF, tH, tT)
            xs = x + t
            P = np.abs(fin0(xs)) + B + tau
            E1 = E + tau + U * P
            mx = np.where(top_ok, xs, -np.inf).max(axis=1, keepdims=True)
            assert np.all(np.isfinite(mx[:, 0, :][act & (tile.nG > 0)[:, None]])), "an evaluation without a finite value"
            xn = xs - np.where(np.isfinite(mx), mx, 0.0)
            hstar = np.where(top_ok, xs, -np.inf).argmax(axis=1)[:, None, :]
            E1h = np.take_along_axis(E1, hstar, axis=1)
            cand = top_ok & np.isfinite(xn) & (xn >= -(E1 + E1h))
            Etop1 = np.where(cand, E1, 0.0).max(axis=1, keepdims=True)
            Q = np.abs(fin0(xn)) + E1 + Etop1
            a3 = act[:, None, :]
            M = np.where(a3 & np.isfinite(xs), np.maximum(M, np.abs(fin0(x)) + np.abs(fin0(t))), M)
            x = np.where(a3, xn, x)
            E = np.where(a3, E1 + U * Q, E)
            B = np.where(a3, E1 + Etop1 + U * Q, B)
    live = tile.live
    return np.where(live, x, np.nan), np.where(live, B, np.nan), np.where(live, M, np.nan)


def gl2_replay(tile):
    """uint32 [site][G][sample]: the bit patterns the reference's float32 recurrence writes, the missing pattern where no value exists"""
    S, N = tile.depth.shape
    G = tile.G
    valid = np.broadcast_to((np.arange(G)[None, :, None] < tile.nG[:, None, None]), (S, G, N))
    g = np.full((S, G, N), -0.0, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(tile.depth.max(initial=0))):
            act, ao, q, e = tile.read(r)
            tt = _terms(q, e, tile.flags, None, tile.per_read)[6:]
            t = _pick(tile.matches(ao), tt[2], tt[1], tt[0])
            a = (g.astype(np.float64) + t).astype(np.float32)
            m = np.where(valid, a, np.float32(-np.inf)).max(axis=1, keepdims=True)
            g = np.where(act[:, None, :], (a - np.where(np.isfinite(m), m, np.float32(0))).astype(np.float32), g)
    return np.where(tile.live, g.view(np.uint32), np.uint32(F32_MISSING_BITS))


def compare_gl(gl_bits, x, B, live):
    """(values, worst |GL - x| / B, misplaced): every live float32 GL against the exact value and its bound; `misplaced` counts a -inf, a
    missing pattern or a NaN that does not stand exactly where the model has it"""
    gl_bits = np.asarray(gl_bits, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        gl = gl_bits.view(np.float32).astype(np.float64)
        bad = int((gl_bits[~live] != F32_MISSING_BITS).sum()) + int((np.isnan(gl[live])).sum())
        inf_model, inf_got = live & np.isneginf(x), live & np.isneginf(gl)
        bad += int((inf_model != inf_got).sum())
        fin = live & np.isfinite(x) & np.isfinite(gl)
        ratio = np.where(fin, np.abs(gl - np.where(fin, x, 0.0)) / np.where(fin, B, 1.0), 0.0)
    return int(live.sum()), float(ratio.max(initial=0.0)), bad


def ulp_distance(a_bits, b_bits):
    """distance in float32 units in the last place between bit patterns of values <= 0 (equal signs: the patterns are ordered)"""
    return np.abs(np.asarray(a_bits, dtype=np.uint32).astype(np.int64) - np.asarray(b_bits, dtype=np.uint32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ GL model 1
_TAIL = {}


def binom_tail_ratios(n, e):
    """[P(X >= k+1) / P(X >= k) for k = 0..n-1] exactly, X ~ Binomial(n, e), e a Fraction"""
    pmf = [Fraction(math.comb(n, j)) * e ** j * (1 - e) ** (n - j) for j in range(n + 1)]
    tail = [Fraction(0)] * (n + 2)
    for j in range(n, -1, -1):
        tail[j] = tail[j + 1] + pmf[j]
    return [tail[k + 1] / tail[k] for k in range(n)]


def gl1_costs(depcorr, codes):
    """codes: qual << 5 | base (strand 0).  Returns the 5x5 matrix of phred-scaled costs (float64):

        beta(q, n, k) = -10 log10( P(X >= k+1) / P(X >= k) ),   X ~ Binomial(n, e),  e = 10^(-q/10)
        fk(w)         = (1 - depcorr)^w (1 - eta) + eta,  eta = 0.03
        reads in descending (quality, base) order; per base b with running count c_b and per (strand, base) count w:
            bsum_b += fk(w) beta(q, n, c_b)
        homozygous j:      sum_{b != j} bsum_b                                   (0 when no other base was seen)
        heterozygous j,k:  -4.343 (ln C(c_j + c_k, c_k) - (c_j + c_k) ln 2) + sum_{b not in {j,k}} bsum_b"""
    n_all = len(codes)
    assert n_all <= 255
    eta = 0.03
    fk = lambda w: (1.0 - depcorr) ** w * (1.0 - eta) + eta
    order = sorted(codes, reverse=True)
    c, w, bsum = [0] * 5, [0] * 5, [0.0] * 5
    for code in order:
        q = min(max(code >> 5, 4), 63)
        b = code & 0xF
        if (q, n_all) not in _TAIL:
            e = Fraction(10.0 ** (-q / 10.0))
            _TAIL[(q, n_all)] = [-10.0 * math.log10(float(r)) for r in binom_tail_ratios(n_all, e)]
        bsum[b] += fk(w[b]) * _TAIL[(q, n_all)][c[b]]
        c[b] += 1; w[b] += 1
    out = np.zeros((5, 5))
    for j in range(5):
        others = [k for k in range(5) if k != j]
        out[j, j] = sum(bsum[k] for k in others) if sum(c[k] for k in others) else 0.0
        for k in range(j + 1, 5):
            rest = [i for i in range(5) if i not in (j, k)]
            cjk = c[j] + c[k]
            lhet = math.log(math.comb(cjk, c[k])) - cjk * math.log(2.0)
            v = -4.343 * lhet + (sum(bsum[i] for i in rest) if sum(c[i] for i in rest) else 0.0)
            out[j, k] = out[k, j] = max(v, 0.0)
        out[j, j] = max(out[j, j], 0.0)
    return out


def gl1_cost_differences(tile, depcorr):
    """GL model 1 on a tile: (want, tol) [site][G][sample] float64 -- cost of the genotype minus the smallest cost of the evaluation
    (-10 GL), from gl1_costs over the evaluation's reads, and the tolerance of that difference when each of the two costs is held to
    rtol 2e-6, atol 1e-4; nan where no value exists.  Evaluations deeper than 255 reads are outside the model (a random subsample)."""
    S, N = tile.depth.shape
    want, tol = np.full((S, tile.G, N), np.nan), np.full((S, tile.G, N), np.nan)
    q_all = gl_scores(tile.reads, tile.read_errp, tile.flags)
    cache = {}
    for s in range(S):
        nA = int(tile.n_alleles[s])
        for n in range(N):
            d = int(tile.depth[s, n])
            if d == 0 or d > 255:
                continue
            codes = tuple(sorted((int(q_all[r, s, n]) << 5) | (int(tile.reads[r, s, n]) & 3) for r in range(d)))
            if codes not in cache:
                cache[codes] = gl1_costs(depcorr, list(codes))
            m = cache[codes]
            c = np.array([m[int(tile.alleles2acgt[s, A1[g]]), int(tile.alleles2acgt[s, A2[g]])] for g in range(nA * (nA + 1) // 2)])
            want[s, : c.size, n] = c - c.min()
            tol[s, : c.size, n] = 2e-4 + 2e-6 * (c + c.min())
    return want, tol


# ------------------------------------------------------------------------------------------------ counts and sums
def counts_from_reads(tile, sum_scores=None, mapq=20):
    """the tags that are sums over the reads, as a dict of integer arrays (allele order, canonical planes):
         dp [S][N]        the reads of the evaluation (fmt_dp at written sites)
         ad [S][A][N]     reads per allele; the unobserved allele and alleles beyond n_alleles: 0
         info_dp [S], info_ad [S][A]    their totals over the samples
         i16 [S][12]      fields 1+2 | 3+4 as (ref count, 0, other count, 0): the strand split is not in the dump; 5-8 quality sum and
                          sum of squares of the reference allele's reads | the others'; 9-12 mapq x count and mapq^2 x count; all 0 at
                          a site with one allele.  "Others" are alleles 1 .. without the unobserved one.
         qs [S][A]        Fractions: sum over samples of qsum[s][allele] / sum_b qsum[s][b], samples without quality mass left out
       sum_scores: the score each read adds to the quality sums, [read][site][sample] (--adjust-qs bit 2: the adjusted one); default
       the raw score of the dump.  The square of a score is capped at 63^2 (QS_TO_QSSQ)."""
    S, N = tile.depth.shape
    A = 5 if tile.G == 15 else 4
    sc = (tile.reads.astype(np.int64) >> 2) if sum_scores is None else np.asarray(sum_scores, dtype=np.int64)
    cnt, qsum, qsq = (np.zeros((S, 4, N), dtype=np.int64) for _ in range(3))
    for r in range(int(tile.depth.max(initial=0))):
        act = r < tile.depth
        base = tile.reads[r].astype(np.int64) & 3
        for b in range(4):
            hit = act & (base == b)
            cnt[:, b, :] += hit
            qsum[:, b, :] += np.where(hit, sc[r], 0)
            qsq[:, b, :] += np.where(hit, np.minimum(sc[r], CAP_BASEQ) ** 2, 0)
    ad = np.zeros((S, A, N), dtype=np.int64)
    i16 = np.zeros((S, 12), dtype=np.int64)
    qs = np.empty((S, A), dtype=object)
    qs[:] = Fraction(0)
    for s in range(S):
        if tile.site_status[s] != SITE_OK:
            continue
        nA = int(tile.n_alleles[s])
        tot = qsum[s].sum(axis=0)
        for a in range(nA):
            b = int(tile.alleles2acgt[s, a])
            if not 0 <= b < 4:
                continue
            ad[s, a] = cnt[s, b]
            qs[s, a] = sum((Fraction(int(qsum[s, b, n]), int(tot[n])) for n in range(N) if tot[n] != 0), Fraction(0))
            if nA > 1:
                o = 0 if a == 0 else 2
                c = int(cnt[s, b].sum())
                i16[s, o] += c
                i16[s, 4 + o] += int(qsum[s, b].sum())
                i16[s, 5 + o] += int(qsq[s, b].sum())
                i16[s, 8 + o] += mapq * c
                i16[s, 9 + o] += mapq * mapq * c
    return dict(dp=tile.depth.copy(), ad=ad, info_dp=tile.depth.sum(axis=1), info_ad=ad.sum(axis=2), i16=i16, qs=qs)


def check_counts(c, got, n_samples):
    """the tags a tile wrote (a dict of canonical arrays: any of fmt_dp, fmt_ad, fmt_adf + fmt_adr as fmt_adfr, info_dp, info_ad,
    info_adf + info_adr as info_adfr, i16, qs) against counts_from_reads' dict: integers equal, I16 1+2 / 3+4 as sums, QS within
    N 2^-24 exact + 2^-149 (one float32 division and at most N - 1 float32 additions of non-negative terms per allele).
    Returns the worst QS error / bound (0.0 without QS)."""
    for name, key in (("fmt_dp", "dp"), ("fmt_ad", "ad"), ("fmt_adfr", "ad"), ("info_dp", "info_dp"), ("info_ad", "info_ad"), ("info_adfr", "info_ad")):
        if name in got:
            assert np.array_equal(np.asarray(got[name]).astype(np.int64), c[key]), name
    if "i16" in got:
        v = np.asarray(got["i16"], dtype=np.float64)
        have = np.stack([v[:, 0] + v[:, 1], v[:, 2] + v[:, 3]] + [v[:, i] for i in range(4, 12)], axis=1)
        want = np.stack([c["i16"][:, 0], c["i16"][:, 2]] + [c["i16"][:, i] for i in range(4, 12)], axis=1)
        assert want.max(initial=0) < 2 ** 24, "a sum beyond the integers float32 holds exactly: choose a smaller shape"
        assert np.array_equal(have, want.astype(np.float64)), "I16 fields 1-12"
    worst = 0.0
    if "qs" in got:
        q = np.asarray(got["qs"], dtype=np.float32)
        for s in range(q.shape[0]):
            for a in range(q.shape[1]):
                ex = c["qs"][s, a]
                r = abs(Fraction(float(q[s, a])) - ex) / (n_samples * Fraction(1, 2 ** 24) * ex + Fraction(1, 2 ** 149))
                worst = max(worst, float(r))
        assert worst <= 1.0, f"QS error / bound {worst:.3f}"
    return worst
