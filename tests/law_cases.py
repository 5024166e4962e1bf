"""The cases of the tile-mode law tests -- TEST INFRASTRUCTURE shared by tests/test_tile_laws_cpu.py (the oracle) and
tests/test_gpu_tile_laws.py (the device).  A case simulates tiles through `run` (the oracle or the device behind one signature),
applies the statistics of laws.py and returns {name: (kind, value)}: kind "z" passes with |value| < 5, kind "chi2" (statistic over
chi2_limit(dof)) with value < 1, kind "exact" (a count of violations) with value == 0.

CASES fixes the order: the seed of a case is 1000 + its index, written down before anything was run."""
import numpy as np

import laws
from vcfgl_amd import VcfglArgs, _abi

MIXED_DEPTHS = (0.3, 5.0, 11.99, 12.0, 20.0, 100.0)

CASES = [
    ("depth-0.3", "depth", 0.3), ("depth-5", "depth", 5.0), ("depth-11.99", "depth", 11.99), ("depth-12", "depth", 12.0),
    ("depth-20", "depth", 20.0), ("depth-100", "depth", 100.0), ("depth-per-sample", "depths", MIXED_DEPTHS),
    ("haplotype", "haplotype", None),
    ("base-error-0.002", "base", 0.002), ("base-error-0.05", "base", 0.05), ("base-error-0.3", "base", 0.3),
    ("read-errp-0.01-1e-05", "errp", (0.01, 1e-5)), ("read-errp-0.05-0.03-alpha-below-1", "errp", (0.05, 0.03)),
    ("read-errp-0.2-0.032", "errp", (0.2, 0.032)), ("read-errp-0.01-1e-09", "errp", (0.01, 1e-9)),
    ("site-error-0.01-1e-05", "site", (0.01, 1e-5)), ("site-error-0.05-0.03-alpha-below-1", "site", (0.05, 0.03)),
    ("tail-distance", "tail", None),
    ("independence", "independence", None),
    # negative controls: overlapped caller layouts that the same statistics must flag
    ("control-stride1-lag1-u", "control", "stride1"), ("control-off1-eq-off2-haplotype-error", "control", "hap_err"),
    ("control-block1-neighbour-depth", "control", "block1"), ("control-off3-eq-off0-depth-u", "control", "depth_u"),
]
SEED = {name: 1000 + i for i, (name, _, _) in enumerate(CASES)}
POSITIVE = [c for c in CASES if c[1] != "control"]
CONTROLS = [c for c in CASES if c[1] == "control"]
CONTROL_Z = 20.0          # a control must reach |z| >= 20


def tile_args(seed, **kw):
    a = VcfglArgs(seed=seed, **kw)
    a.rng_mode, a.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    return a


def hom_sites(S, N):
    return np.zeros((S, N), dtype=np.uint8)                        # A/A


def het_sites(S, N):
    """A/C and C/A alternating over the samples and sites: allele 0 is A where site + sample is even"""
    odd = (np.arange(S)[:, None] + np.arange(N)[None, :]) & 1
    return np.where(odd, 0x01, 0x10).astype(np.uint8)


def base_counts(t, base):
    """FORMAT/AD [S][N] of one ACGT base: the planes come in the site's allele order (alleles2acgt)"""
    ad, a2b = t.numpy("fmt_ad"), t.numpy("alleles2acgt")
    out = np.zeros((ad.shape[0], ad.shape[2]), dtype=np.int64)
    for a in range(ad.shape[1]):
        here = a2b[:, a] == base
        out[here] = np.maximum(ad[here, a, :], 0)
    return out


def live_reads(t, cap):
    dp = t.numpy("fmt_dp")
    assert int(dp.max()) <= cap, "a depth beyond the dump's rows"
    return np.arange(cap)[:, None, None] < dp[None, :, :]


def default_layout(args, N):
    import ctypes as C
    p, _keep = args.to_struct(N)
    lay = _abi.RngLayout()
    assert _abi.load_library().vgl_default_rng_layout(C.byref(p), C.byref(lay)) == 0
    return lay.block, [lay.off[k] for k in range(4)], lay.qs_read_stride


# ------------------------------------------------------------------------------------------------------------------ the laws
def depth_stats(dp, lam, tag=""):
    dp = np.asarray(dp).ravel()
    K = int(lam + 12.0 * np.sqrt(lam) + 20.0)
    pmf = laws.poisson_pmf(np.arange(K), lam)
    probs = np.append(pmf, max(0.0, 1.0 - pmf.sum()))
    counts = np.bincount(np.minimum(dp, K), minlength=K + 1)
    zm, zv = laws.poisson_mean_var_z(dp, lam)
    return {f"depth{tag} pmf": ("chi2", laws.chi2_ratio(counts, probs)), f"depth{tag} mean": ("z", zm), f"depth{tag} variance": ("z", zv)}


def case_depth(run, seed, lam, S, N):
    t = run(tile_args(seed, depth=lam, error_rate=0.01), hom_sites(S, N), fields=["fmt_dp"])
    return depth_stats(t.numpy("fmt_dp"), lam)


def case_depths(run, seed, lams, S, N):
    depths = [lams[s % len(lams)] for s in range(N)]
    t = run(tile_args(seed, depth=None, depths=depths, error_rate=0.01), hom_sites(S, N), fields=["fmt_dp"])
    dp, out = t.numpy("fmt_dp"), {}
    for g, lam in enumerate(lams):
        out.update(depth_stats(dp[:, g::len(lams)], lam, tag=f"[{lam}]"))
    return out


def case_haplotype(run, seed, S, N):
    """heterozygous sites, e = 0: the C count of an evaluation is Binomial(depth, 1/2)"""
    t = run(tile_args(seed, depth=8.0, error_rate=0.0, add_fmt_ad=1), het_sites(S, N), fields=["fmt_dp", "fmt_ad"])
    d, k = t.numpy("fmt_dp").astype(np.int64), base_counts(t, 1)
    assert np.array_equal(k + base_counts(t, 0), d)
    return {"haplotype total": ("z", laws.binom_z(int(k.sum()), int(d.sum()), 0.5)), "haplotype dispersion": ("z", laws.dispersion_z(k, d, 0.5))}


def case_base(run, seed, e, S, N):
    """homozygous A/A sites: wrong bases Binomial(reads, e), uniform over C, G, T; strands 1/2 each (vcfgl.cpp:582)"""
    cap = 32
    t = run(tile_args(seed, depth=6.0, error_rate=e, add_fmt_adf=1, add_fmt_adr=1), hom_sites(S, N), fields=["fmt_dp", "fmt_adf", "fmt_adr"], read_capacity=cap)
    live = live_reads(t, cap)
    base = (t.numpy("reads") & 3)[live]
    total, by_base = base.size, np.bincount(base, minlength=4)
    fwd, rev = int(np.maximum(t.numpy("fmt_adf"), 0).sum()), int(np.maximum(t.numpy("fmt_adr"), 0).sum())
    assert fwd + rev == total
    return {"wrong-base count": ("z", laws.binom_z(int(by_base[1:].sum()), total, e)),
            "wrong-base identity": ("chi2", laws.chi2_ratio(by_base[1:], [1 / 3, 1 / 3, 1 / 3])),
            "strand": ("z", laws.binom_z(fwd, total, 0.5))}


def beta_stats(p, mean, var, tag):
    a, b = laws.beta_shape(mean, var)
    m, v, mu4 = laws.beta_moments(a, b)
    u = laws.betainc(a, b, p)
    counts = np.bincount(np.minimum((u * 64.0).astype(np.int64), 63), minlength=64)
    return {f"{tag} u histogram": ("chi2", laws.chi2_ratio(counts, np.full(64, 1 / 64))),
            f"{tag} mean": ("z", laws.mean_z(p, m, v)), f"{tag} variance": ("z", laws.var_z(p, m, v, mu4))}


def case_errp(run, seed, shape, S, N):
    cap = 32
    mean, var = shape
    t = run(tile_args(seed, depth=4.0, error_rate=mean, error_qs=2, beta_variance=var), hom_sites(S, N), fields=["fmt_dp"], read_capacity=cap, deviates=True)
    live = live_reads(t, cap)
    p = t.numpy("read_errp")[live]
    out = beta_stats(p, mean, var, "read error probability")
    out["staged quality score"] = ("exact", int((laws.qscore_of(p) != (t.numpy("reads")[live] >> 2)).sum()))
    return out


def case_site(run, seed, shape, S, N):
    assert N == 1
    mean, var = shape
    t = run(tile_args(seed, depth=5.0, error_rate=mean, error_qs=1, beta_variance=var, add_info_dp=1), hom_sites(S, 1), fields=["fmt_dp", "info_dp"], deviates=True)
    p = t.numpy("site_pick_err")[t.numpy("info_dp") > 0]
    return beta_stats(p, mean, var, "site error rate")


def case_tail(run, seed, S, N):
    assert N == 1
    t = run(tile_args(seed, depth=1.0, error_rate=0.01, add_i16=1, add_info_dp=1), hom_sites(S, 1), fields=["fmt_dp", "info_dp", "i16"])
    one = t.numpy("info_dp") == 1
    i16 = t.numpy("i16")[one].astype(np.float64)
    td, sq = i16[:, 12] + i16[:, 14], i16[:, 13] + i16[:, 15]
    ok = (td == np.rint(td)) & (td >= 1) & (td <= 25) & (sq == td * td)
    counts = np.bincount(td.astype(np.int64), minlength=26)[:26]
    return {"tail distance histogram": ("chi2", laws.chi2_ratio(counts[1:], laws.tail_pmf()[1:])), "tail distance squares": ("exact", int((~ok).sum()))}


# ------------------------------------------------------------------------------------------------------------------ independence
INDEP_BETA = (0.05, 1e-4)


class ReadTile:
    """per-evaluation summaries of a tile with a per-read dump at heterozygous sites: depth, bases that are neither allele, u of every read"""
    CAP = 32

    def __init__(self, run, args, S, N, site0):
        gt = het_sites(S, N)
        t = run(args, gt, site0=site0, fields=["fmt_dp"], read_capacity=self.CAP, deviates=True)
        self.dp = t.numpy("fmt_dp").astype(np.int64)
        self.live = live_reads(t, self.CAP)
        self.base = t.numpy("reads") & 3
        self.wrong = (self.live & (self.base >= 2)).sum(axis=0)
        a, b = laws.beta_shape(args.error_rate, args.beta_variance)
        self.u = np.zeros(self.live.shape)
        self.u[self.live] = laws.betainc(a, b, t.numpy("read_errp")[self.live])
        self.a0 = gt & 15


def hap_error_z(rt):
    """read 0 of a heterozygous evaluation: the haplotype draw against the error draw.  An error hides the haplotype, so the pair is seen through
    its symmetry: independent draws show allele 0 and allele 1 equally often ((1 - e) / 2 + e / 6 each, vcfgl.cpp:473,486-488), whatever e is;
    an error test that shares the haplotype's uniform puts every error on one allele (allele 0: 1/2 - e against 1/2 + e / 3).  Binomial z of
    'shows allele 0' among the reads 0 that show either allele."""
    has = rt.dp >= 1
    b0 = rt.base[0][has]
    a0 = rt.a0[has]
    either = b0 < 2
    return laws.binom_z(int((b0[either] == a0[either]).sum()), int(either.sum()), 0.5)


def lag_u_z(rt, lag):
    x, y = rt.u[:-lag], rt.u[lag:]
    both = rt.live[lag:]                                         # read r + lag exists => read r exists
    return laws.corr_z(x[both], y[both])


def depth_u_z(rt):
    has = rt.dp >= 1
    return laws.corr_z(rt.dp[has], rt.u[0][has])


def pair_stats(tag, A, B, sel_a, sel_b):
    """depth, wrong-base count and u of read 0 of paired evaluations (A[sel_a] with B[sel_b])"""
    out = {f"{tag}: depth": ("z", laws.corr_z(A.dp[sel_a], B.dp[sel_b])), f"{tag}: wrong-base count": ("z", laws.corr_z(A.wrong[sel_a], B.wrong[sel_b]))}
    both = (A.dp[sel_a] >= 1) & (B.dp[sel_b] >= 1)
    out[f"{tag}: u of read 0"] = ("z", laws.corr_z(A.u[0][sel_a][both], B.u[0][sel_b][both]))
    return out


def independence_args(seed, layout=None, depth=6.0):
    return tile_args(seed, depth=depth, error_rate=INDEP_BETA[0], error_qs=2, beta_variance=INDEP_BETA[1], rng_layout=layout)


def case_independence(run, seed, S, N):
    args = independence_args(seed)
    site0 = 3
    T = ReadTile(run, args, S, N, site0)
    out = {}
    out.update(pair_stats("sample j, j+1", T, T, np.s_[:, :-1], np.s_[:, 1:]))
    out.update(pair_stats("site s, s+1", T, T, np.s_[:-1, :], np.s_[1:, :]))
    out["reads r, r+1: u"] = ("z", lag_u_z(T, 1))
    out["reads r, r+2: u"] = ("z", lag_u_z(T, 2))
    out["one evaluation: depth, u of read 0"] = ("z", depth_u_z(T))
    out["one evaluation: haplotype, error of read 0"] = ("z", hap_error_z(T))
    for k in (10, 16):
        B = ReadTile(run, args, S, N, site0 + (1 << k))
        out.update(pair_stats(f"site s, s+2^{k}", T, B, np.s_[:, :], np.s_[:, :]))
        del B
    return out


# ------------------------------------------------------------------------------------------------------------------ negative controls
def case_control(run, seed, which, S, N):
    if which == "block1":                                        # neighbouring samples one draw apart
        args = tile_args(seed, depth=20.0, error_rate=0.01)
        _, off, stride = default_layout(args, N)
        args.rng_layout = (1, off, stride)
        dp = run(args, hom_sites(S, N), site0=3, fields=["fmt_dp"]).numpy("fmt_dp")
        return {"sample j, j+1: depth": ("z", laws.corr_z(dp[:, :-1], dp[:, 1:]))}
    args = independence_args(seed)
    block, off, stride = default_layout(args, N)
    if which == "stride1":
        args.rng_layout = (block, off, 1)
    elif which == "hap_err":
        args.rng_layout = (block, [off[0], off[1], off[1], off[3]], stride)
    elif which == "depth_u":
        args.rng_layout = (block, [off[0], off[1], off[2], off[0]], stride)
    T = ReadTile(run, args, S, N, 3)
    stat = {"stride1": lambda: lag_u_z(T, 1), "hap_err": lambda: hap_error_z(T), "depth_u": lambda: depth_u_z(T)}[which]()
    name = {"stride1": "reads r, r+1: u", "hap_err": "one evaluation: haplotype, error of read 0", "depth_u": "one evaluation: depth, u of read 0"}[which]
    return {name: ("z", stat)}


def run_case(run, name, kind, param, S, N):
    seed = SEED[name]
    if kind in ("haplotype", "tail", "independence"):
        return {"haplotype": case_haplotype, "tail": case_tail, "independence": case_independence}[kind](run, seed, S, N)
    return {"depth": case_depth, "depths": case_depths, "base": case_base, "errp": case_errp, "site": case_site, "control": case_control}[kind](run, seed, param, S, N)


def report(name, stats):
    """one line per statistic (the figures of the comment blocks at the top of the two test files come from these)"""
    for k, (kind, v) in stats.items():
        print(f"LAW {name} | {k} | {kind} | {v:.4g}")


def assert_inside(name, stats):
    report(name, stats)
    for k, (kind, v) in stats.items():
        if kind == "z":
            assert abs(v) < laws.Z_LIMIT, (name, k, v)
        elif kind == "chi2":
            assert v < 1.0, (name, k, "chi-square over its limit", v)
        else:
            assert v == 0, (name, k, v)
