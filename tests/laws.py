"""Exact laws of the reference's samplers and the statistics that test draws against them -- TEST INFRASTRUCTURE.

Every statistic is written once here and applied by tests/test_tile_laws_cpu.py (the oracle) and tests/test_gpu_tile_laws.py (the
device).  Only `math` and `numpy`.  The limits are conditions fixed before anything is run: |z| < Z_LIMIT for every z statistic
and chi2_limit(dof) for every chi-square, the Wilson-Hilferty quantile at the same z -- about 3e-7 per statistic.

The laws (reference lines):
  depth            Poisson(lambda): product method below 12, rejection method from 12 on            rng.h:284-351
  haplotype        each read takes allele 0 with probability 1/2                                    vcfgl.cpp:473
  base error       with probability e the base is redrawn uniformly among the three others          vcfgl.cpp:486-488
  strand           forward with probability 1/2                                                     vcfgl.cpp:582
  error probability Beta(alpha, beta), alpha = ((1 - m) / v - 1 / m) m^2, beta = alpha (1 / m - 1)  rng.h:455-460 (:368-371)
                   from m = --error-rate and v = --beta-variance                                    io.cpp:1036-1043
  quality score    (int)(-10 log10 p), capped at 63; 63 for p == 0, 0 for p == 1                    vcfgl.cpp:500-523
  tail distance    min(1 + x / (RAND_MAX / 50 + 1), 25), x uniform on [0, 2^31)                     rng.h:12, vcfgl.cpp:647-663
"""
import math

import numpy as np

Z_LIMIT = 5.0
_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def lgamma(x):
    return np.asarray(_lgamma(np.asarray(x, dtype=np.float64)), dtype=np.float64)


# ---------------------------------------------------------------------------------------------- probability mass functions
def poisson_pmf(k, lam):
    k = np.asarray(k, dtype=np.float64)
    if lam == 0.0:
        return (k == 0).astype(np.float64)
    return np.exp(k * math.log(lam) - lam - lgamma(k + 1.0))


def binom_pmf(k, n, p):
    k = np.asarray(k, dtype=np.float64)
    return np.exp(lgamma(n + 1.0) - lgamma(k + 1.0) - lgamma(n - k + 1.0) + k * math.log(p) + (n - k) * math.log1p(-p))


def tail_pmf():
    """P(t), t = 0 .. 25, of one tail distance: 50 equal cells of [0, 2^31) capped at 25 (the 50th cell is two values short)"""
    cell = 2147483647 // 50 + 1
    w = np.array([min(cell, (1 << 31) - c * cell) for c in range(50)], dtype=np.float64) / float(1 << 31)
    p = np.zeros(26)
    p[1:25] = w[:24]
    p[25] = w[24:].sum()
    return p


# ---------------------------------------------------------------------------------------------- the beta law
def beta_shape(mean, var):
    """(alpha, beta) exactly as the reference derives them (rng.h:456-460)"""
    oom = 1.0 / mean
    a = (((1.0 - mean) / var) - oom) * mean ** 2
    return a, a * (oom - 1.0)


def beta_moments(a, b):
    """mean, variance and fourth central moment of Beta(a, b)"""
    s = a + b
    var = a * b / (s * s * (s + 1.0))
    exk = 6.0 * ((a - b) ** 2 * (s + 1.0) - a * b * (s + 2.0)) / (a * b * (s + 2.0) * (s + 3.0))
    return a / s, var, (exk + 3.0) * var * var


def _betacf(a, b, x):
    """continued fraction of the incomplete beta function by the modified Lentz method (float64), elementwise over x; an element
    leaves the iteration once its factor is 1 to 1e-16"""
    tiny = 1e-300
    n = x.size
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones(n)
    d = 1.0 - qab * x / qap
    d[np.abs(d) < tiny] = tiny
    d = 1.0 / d
    h = d.copy()
    out = np.empty(n)
    idx = np.arange(n)
    for m in range(1, 200000):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d[np.abs(d) < tiny] = tiny
        c = 1.0 + aa / c
        c[np.abs(c) < tiny] = tiny
        d = 1.0 / d
        h = h * d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d[np.abs(d) < tiny] = tiny
        c = 1.0 + aa / c
        c[np.abs(c) < tiny] = tiny
        d = 1.0 / d
        de = d * c
        h = h * de
        done = np.abs(de - 1.0) <= 1e-16
        if done.any():
            out[idx[done]] = h[done]
            keep = ~done
            if not keep.any():
                return out
            idx, x, c, d, h = idx[keep], x[keep], c[keep], d[keep], h[keep]
    raise ArithmeticError("incomplete beta: the continued fraction did not converge")


def betainc(a, b, x):
    """regularised incomplete beta function I_x(a, b) = F_Beta(a,b)(x), elementwise over x in [0, 1]"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out = np.zeros(x.shape)
    out[x >= 1.0] = 1.0
    inside = (x > 0.0) & (x < 1.0)
    xi = x[inside]
    if xi.size:
        lbt = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * np.log(xi) + b * np.log1p(-xi)
        direct = xi < (a + 1.0) / (a + b + 2.0)
        r = np.empty(xi.size)
        if direct.any():
            r[direct] = np.exp(lbt[direct]) * _betacf(a, b, xi[direct]) / a
        if (~direct).any():
            r[~direct] = 1.0 - np.exp(lbt[~direct]) * _betacf(b, a, 1.0 - xi[~direct]) / b
        out[inside] = r
    return out


def qscore_of(p):
    """the staged quality score of an error probability, the reference's rule without --qs-bins (vcfgl.cpp:500-523)"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, 63, dtype=np.int64)
    mid = (p > 0.0) & (p < 1.0)
    q[mid] = np.minimum((-10.0 * np.log10(p[mid])).astype(np.int64), 63)
    q[p == 1.0] = 0
    return q


# ---------------------------------------------------------------------------------------------- statistics
def chi2_limit(dof):
    """Wilson-Hilferty quantile of chi-square(dof) at z = 5"""
    t = 2.0 / (9.0 * dof)
    return dof * (1.0 - t + Z_LIMIT * math.sqrt(t)) ** 3


def chi2_gof(counts, probs):
    """(statistic, degrees of freedom) of observed counts against cell probabilities that sum to 1; cells that expect fewer than
    10 counts are merged into one (and that one, while it still expects fewer than 10, with the smallest cell that is left)"""
    counts = np.asarray(counts, dtype=np.float64).ravel()
    probs = np.asarray(probs, dtype=np.float64).ravel()
    assert counts.shape == probs.shape and abs(probs.sum() - 1.0) < 1e-9, ("cell probabilities must sum to 1", probs.sum())
    n = counts.sum()
    exp = n * probs
    small = exp < 10.0
    o, e = list(counts[~small]), list(exp[~small])
    if small.any():
        po, pe = counts[small].sum(), exp[small].sum()
        while pe < 10.0 and e:
            j = int(np.argmin(e))
            po, pe = po + o.pop(j), pe + e.pop(j)
        o.append(po)
        e.append(pe)
    o, e = np.array(o), np.array(e)
    assert len(e) >= 2, "fewer than two cells after merging"
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


def chi2_ratio(counts, probs):
    """chi-square statistic over its limit: a case passes below 1"""
    stat, dof = chi2_gof(counts, probs)
    return stat / chi2_limit(dof)


def mean_z(x, mean, var):
    """z of the sample mean of draws with the given mean and variance"""
    x = np.asarray(x, dtype=np.float64)
    return float((x.mean() - mean) * math.sqrt(x.size / var))


def var_z(x, mean, var, mu4):
    """z of the mean squared deviation from the KNOWN mean: expectation var, variance (mu4 - var^2) / n"""
    x = np.asarray(x, dtype=np.float64)
    return float((((x - mean) ** 2).mean() - var) * math.sqrt(x.size / (mu4 - var * var)))


def poisson_mean_var_z(k, lam):
    """(z of the mean, z of the variance) of Poisson(lam) draws: fourth central moment lam + 3 lam^2"""
    return mean_z(k, lam, lam), var_z(k, lam, lam, lam + 3.0 * lam * lam)


def binom_z(k, n, p):
    """z of a total of k successes in n trials of probability p"""
    return float((k - n * p) / math.sqrt(n * p * (1.0 - p)))


def dispersion_z(k, d, p=0.5):
    """z of sum_i (k_i - d_i p)^2 / (d_i p q) over the evaluations with d_i > 0, k_i ~ Binomial(d_i, p): each term has expectation 1 and
    variance 2 - 6 / d_i + 1 / (d_i p q) (fourth central moment of the binomial: d p q (1 + 3 (d - 2) p q)).  Reads of one evaluation
    that move together push it up, reads that avoid one another push it down."""
    k, d = np.asarray(k, dtype=np.float64).ravel(), np.asarray(d, dtype=np.float64).ravel()
    k, d = k[d > 0], d[d > 0]
    pq = p * (1.0 - p)
    x = ((k - d * p) ** 2 / (d * pq)).sum()
    v = (2.0 - 6.0 / d + 1.0 / (d * pq)).sum()
    return float((x - d.size) / math.sqrt(v))


def corr_z(x, y):
    """r sqrt(n) of two paired samples: N(0, 1) when they are independent"""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    assert x.size == y.size and x.size > 2
    x, y = x - x.mean(), y - y.mean()
    den = math.sqrt(float((x * x).sum()) * float((y * y).sum()))
    assert den > 0.0, "a constant sample has no correlation"
    return float((x * y).sum() / den * math.sqrt(x.size))
