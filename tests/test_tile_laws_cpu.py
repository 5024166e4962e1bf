"""VGL_RNG_TILE against the EXACT laws of the reference's samplers, on the CPU oracle.

The parity tests compare the device with the oracle, and the oracle restates the same window specification (include/vcfgl_hip.h,
vgl_rng_layout): windows that overlap or streams that share draws would pass all of them.  Here the oracle's tile-mode output is
tested against the distributions themselves (laws.py cites the reference lines) and for independence between samples, sites,
reads and streams; tests/test_gpu_tile_laws.py runs the same cases (law_cases.py) on the device at twenty times the size.  The
negative controls run the same statistics on caller layouts that overlap on purpose: every one must fire, or the positive cases
would prove nothing.  The last test counts how far consumers step into their windows (DESIGN.md section 2 quotes it).

Limits are conditions, not measurements: |z| < 5, chi-square < chi2_limit(dof) (the Wilson-Hilferty quantile at z = 5), controls
|z| >= 20; seeds are 1000 + the case's index in law_cases.CASES, fixed before the first run.

Observed (about 1e5 evaluations per case; 87 statistics: 60 z, 22 chi-square, 5 exact counts), every positive case at its first seed:
  worst |z|                 2.39   (independence: haplotype against error of read 0)
  worst chi-square / limit  0.54   (site-error-0.01-1e-05: histogram of u)
  controls, |z|             21.9 (stride 1), 22.5 (off[1] = off[2]), 43.1 (block 1), 58.0 (off[3] = off[0])"""
import numpy as np
import pytest

import law_cases as lc

# (sites, samples) per kind of case: about 1e5 evaluations, less where every evaluation carries many reads
SHAPE = {"depth": (2000, 50), "depths": (2000, 48), "haplotype": (2000, 50), "base": (2000, 50), "errp": (1000, 50), "site": (2000, 1),
         "tail": (20000, 1), "independence": (2000, 50), "control": (2000, 50)}


def assert_inside_windows(o, args, N):
    """what is certain about the windows of the default layout: the depth, haplotype and base streams of an evaluation stay inside their
    sub-windows, and the haplotype stream takes exactly one draw per read (FORMAT/DP of them)"""
    mx, hap_diff, hist = o.census()
    _, off, _ = lc.default_layout(args, N)
    assert hap_diff == 0
    for k in range(3):
        assert mx[k] <= off[k + 1] - off[k], (k, mx[k], off)
    return mx, hist


@pytest.fixture(scope="module")
def run(oracle):
    def run_(args, gt, site0=0, fields=None, read_capacity=0, deviates=False):
        o = oracle.Oracle(args, gt.shape[1])
        o.census_begin()
        t = o.simulate(site0, gt, fields=fields, read_capacity=read_capacity, deviates=deviates)
        if args.rng_layout is None:                                # every positive case doubles as a window census
            assert_inside_windows(o, args, gt.shape[1])
        o.close()
        return t
    return run_


@pytest.mark.parametrize("name,kind,param", lc.POSITIVE, ids=[c[0] for c in lc.POSITIVE])
def test_oracle_tile_mode_follows_the_exact_law(run, name, kind, param):
    S, N = SHAPE[kind]
    if name == "depth-100":
        S //= 4                                                    # 100 reads per evaluation
    lc.assert_inside(name, lc.run_case(run, name, kind, param, S, N))


@pytest.mark.parametrize("name,kind,param", lc.CONTROLS, ids=[c[0] for c in lc.CONTROLS])
def test_overlapped_caller_layout_is_flagged(run, name, kind, param):
    S, N = SHAPE[kind]
    stats = lc.run_case(run, name, kind, param, S, N)
    lc.report(name, stats)
    for k, (_, z) in stats.items():
        assert abs(z) >= lc.CONTROL_Z, (name, k, z)


@pytest.mark.parametrize("shape", ["C3", "alpha-below-1"])
def test_window_census(oracle, shape):
    """include/vcfgl_hip.h: a consumer that needs more draws than its sub-window "simply keeps stepping".  Streams 0-2 never do (asserted);
    a beta deviate of stream 3 that takes more than qs_read_stride = 32 draws steps into the window of the next read: that fraction is
    printed, not bounded (DESIGN.md section 2 quotes it from 2.2e6 deviates per shape)."""
    mean, var = {"C3": (0.01, 1e-5), "alpha-below-1": (0.05, 0.03)}[shape]
    args = lc.tile_args(42, depth=20.0, error_rate=mean, error_qs=2, beta_variance=var)
    N, S = 1000, 10
    o = oracle.Oracle(args, N)
    o.census_begin()
    t = o.simulate(0, lc.hom_sites(S, N), fields=["fmt_dp"])
    mx, hist = assert_inside_windows(o, args, N)
    n = int(hist.sum())
    assert n == int(t.numpy("fmt_dp").sum()) and hist[:6].sum() == 0          # one deviate per read; two gamma deviates take at least six draws
    assert int((hist * np.arange(hist.size)).sum()) >= 6 * n
    block, off, stride = lc.default_layout(args, N)
    assert mx[3] >= stride * (int(t.numpy("fmt_dp").max()) - 1) + 6             # the last read of the deepest evaluation starts at r stride
    print(f"CENSUS {shape}: {n} deviates, {int(hist[stride + 1:].sum())} above {stride} draws, most draws {int(np.nonzero(hist)[0][-1])}, streams reach {mx}")
