"""laws.py against closed forms: the statistics of the tile-mode law tests must themselves be right."""
import math

import numpy as np
import pytest

import laws


def test_pmfs_sum_to_one_and_have_the_right_moments():
    for lam in (0.3, 5.0, 11.99, 12.0, 20.0, 100.0):
        k = np.arange(int(lam + 40 * math.sqrt(lam) + 60))
        p = laws.poisson_pmf(k, lam)
        assert abs(p.sum() - 1.0) < 1e-12 and abs((p * k).sum() - lam) < 1e-10 * max(lam, 1.0)
        assert abs((p * (k - lam) ** 4).sum() - (lam + 3 * lam * lam)) < 1e-8 * lam * lam + 1e-9
    assert list(laws.poisson_pmf(np.arange(3), 0.0)) == [1.0, 0.0, 0.0]
    for n, q in ((1, 0.5), (7, 0.002), (30, 0.3), (255, 0.5)):
        k = np.arange(n + 1)
        p = laws.binom_pmf(k, n, q)
        assert abs(p.sum() - 1.0) < 1e-12 and abs((p * k).sum() - n * q) < 1e-10 * n
        assert abs((p * (k - n * q) ** 4).sum() - n * q * (1 - q) * (1 + 3 * (n - 2) * q * (1 - q))) < 1e-9 * n * n
    t = laws.tail_pmf()
    assert abs(t.sum() - 1.0) < 1e-15 and t[0] == 0.0 and abs(t[25] - 26 / 50) < 1e-8 and np.all(np.abs(t[1:25] - 1 / 50) < 1e-8)


def test_incomplete_beta_against_elementary_cdfs():
    x = np.concatenate([[0.0, 1e-300, 1e-12, 1.0 - 1e-12, 1.0], np.linspace(0.001, 0.999, 997)])
    assert np.abs(laws.betainc(1.0, 1.0, x) - x).max() < 1e-14                                   # uniform
    assert np.abs(laws.betainc(2.0, 1.0, x) - x * x).max() < 1e-14                               # F = x^2
    assert np.abs(laws.betainc(1.0, 2.0, x) - (1.0 - (1.0 - x) ** 2)).max() < 1e-14
    arcsine = np.where(x < 0.5, 2.0 / math.pi * np.arcsin(np.sqrt(x)), 1.0 - 2.0 / math.pi * np.arcsin(np.sqrt(1.0 - x)))
    assert np.abs(laws.betainc(0.5, 0.5, x) - arcsine).max() < 1e-13                             # arcsine law
    # I_x(a, b) = 1 - I_(1-x)(b, a), and the binomial tail: I_p(k, n - k + 1) = P(Binomial(n, p) >= k)
    # (the last shape is --error-rate 0.01 --beta-variance 1e-9: its log-gamma terms are 1e8 and carry 1e-8 of rounding into the prefactor)
    for a, b, tol in ((9.89, 979.1, 1e-12), (0.0292, 0.554, 1e-12), (0.8, 3.2, 1e-12), (98999.99, 9800999.0, 1e-6)):
        xs = np.clip(np.linspace(0.2, 1.8, 41) * a / (a + b), 1e-9, 1 - 1e-9)
        assert np.abs(laws.betainc(a, b, xs) + laws.betainc(b, a, 1.0 - xs) - 1.0).max() < tol
        assert np.all(np.diff(laws.betainc(a, b, xs)) >= 0.0)
    mid = laws.betainc(98999.99, 9800999.0, [98999.99 / (98999.99 + 9800999.0)])[0]
    assert abs(mid - 0.5) < 1e-3                                                                 # nearly normal: the median is the mean
    for n, k, p in ((20, 3, 0.1), (100, 50, 0.5), (255, 2, 0.002)):
        tail = laws.binom_pmf(np.arange(k, n + 1), n, p).sum()
        assert abs(laws.betainc(k, n - k + 1, [p])[0] - tail) < 1e-12


def test_incomplete_beta_against_scipy():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(5)
    for a, b in ((9.89, 979.1), (0.0292, 0.554), (0.8, 3.2), (23.7, 450.0), (1.0, 1.0), (300.0, 2.0)):
        x = np.concatenate([rng.beta(a, b, 500), rng.random(200)])
        assert np.abs(laws.betainc(a, b, x) - special.betainc(a, b, x)).max() < 1e-12


def test_beta_shape_and_moments():
    for mean, var in ((0.01, 1e-5), (0.05, 0.03), (0.2, 0.032), (0.01, 1e-9)):
        a, b = laws.beta_shape(mean, var)
        m, v, mu4 = laws.beta_moments(a, b)
        assert a > 0 and b > 0 and abs(m - mean) < 1e-12 * mean and abs(v - var) < 1e-9 * var
    assert laws.beta_shape(0.05, 0.03)[0] < 1.0                                                  # the alpha < 1 shape of the law tests
    m, v, mu4 = laws.beta_moments(1.0, 1.0)
    assert abs(m - 0.5) < 1e-15 and abs(v - 1 / 12) < 1e-15 and abs(mu4 - 1 / 80) < 1e-15         # uniform
    m, v, mu4 = laws.beta_moments(0.5, 0.5)
    assert abs(v - 1 / 8) < 1e-15 and abs(mu4 - 3 / 128) < 1e-15                                 # arcsine


def test_quality_score_rule():
    p = np.array([0.0, 1.0, 0.1, 0.0999, 0.5, 1e-7, 10 ** -6.3, 0.999])
    assert list(laws.qscore_of(p)) == [63, 0, 10, 10, 3, 63, 63, 0]


def test_chi2_limit_and_merging():
    for dof in (2, 24, 63):
        t = 2.0 / (9.0 * dof)
        assert laws.chi2_limit(dof) == dof * (1 - t + 5 * math.sqrt(t)) ** 3
    # the exact chi-square quantiles at z = 5 (2.87e-7) are 30.13, 75.73 and 135.87
    assert abs(laws.chi2_limit(2) - 33.38) < 0.01 and abs(laws.chi2_limit(24) - 76.53) < 0.01 and abs(laws.chi2_limit(63) - 136.32) < 0.01
    stat, dof = laws.chi2_gof([50, 50, 0, 0], [0.45, 0.45, 0.05, 0.05])                          # 5 + 5 expected: one merged cell of 10
    assert dof == 2 and abs(stat - (25 / 45 * 2 + 10.0)) < 1e-12
    stat, dof = laws.chi2_gof([48, 48, 4], [0.47, 0.47, 0.06])                                   # 6 expected: merged into a neighbour
    assert dof == 1
    assert laws.chi2_gof([100, 100], [0.5, 0.5]) == (0.0, 1)


def test_z_statistics_on_constructed_samples():
    x = np.arange(1000.0)
    assert abs(laws.corr_z(x, 3 * x + 1) - math.sqrt(1000)) < 1e-9 and abs(laws.corr_z(x, -x) + math.sqrt(1000)) < 1e-9
    assert abs(laws.corr_z(np.tile([0.0, 1.0, 0.0, 1.0], 50), np.tile([0.0, 0.0, 1.0, 1.0], 50))) < 1e-12
    assert laws.binom_z(60, 100, 0.5) == 2.0
    assert laws.mean_z(np.array([1.0, 3.0]), 1.0, 2.0) == 1.0
    # every evaluation of depth 4 shows 2 + 2: no spread at all; all 4 + 0: four times the binomial spread
    d = np.full(400, 4)
    assert abs(laws.dispersion_z(np.full(400, 2), d) - (0 - 400) / math.sqrt(400 * 1.5)) < 1e-9
    assert abs(laws.dispersion_z(np.tile([0, 4], 200), d) - (1600 - 400) / math.sqrt(400 * 1.5)) < 1e-9
    assert laws.dispersion_z(np.array([0, 1, 0, 0]), np.array([1, 1, 0, 2])) == (1 + 1 + 2 - 3) / math.sqrt(0 + 0 + 1.0)
    # exact enumeration: the variance of a term is what the statistic assumes
    for dd, q in ((1, 0.5), (3, 0.5), (7, 0.3)):
        k = np.arange(dd + 1)
        w = laws.binom_pmf(k, dd, q)
        term = (k - dd * q) ** 2 / (dd * q * (1 - q))
        assert abs((w * term).sum() - 1.0) < 1e-12
        assert abs((w * (term - 1.0) ** 2).sum() - (2.0 - 6.0 / dd + 1.0 / (dd * q * (1 - q)))) < 1e-12
