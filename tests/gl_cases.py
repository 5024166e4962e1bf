"""The case table of the GL tile tests -- TEST INFRASTRUCTURE shared by test_gpu_gl_tail.py, test_gpu_gl_body.py and
test_gl_body_model_cpu.py: which flags reach which build of the GL kernels, at which shapes, and what each case must produce."""
import math

import numpy as np

import gl_tail_model as M
from vcfgl_amd import VcfglArgs, _abi

SITES = {1: 33, 5: 29, 63: 17, 65: 9, 130: 7}
BETA = dict(error_qs=2, beta_variance=1e-5)
# name: (flags, which build: (fused, gl_wpb, hooks env), layouts, sample counts, fields beyond the standard ones, what must occur)
#   occur: "alleles" -> the n_alleles values that must all be seen at N >= 63 (N = 1: a single sample shows at most two alleles);
#          "inf" -inf next to 0; "cap" a PL of 255; "sub" a GL in (-45.15, -37.93): 10^GL a float32 subnormal; "skip" a skipped site
PATHS = {
    # k_gl<4, 2, false>: -doUnobserved 0, one to four alleles per site (NG 1, 3, 6, 10); -addQS keeps N = 130 off the fused build
    "k_gl-A4": (dict(seed=21, depth=6.0, error_rate=0.001, do_unobserved=0, add_qs=1), (0, 8, None), (0, 1), (1, 63, 65, 130), dict(alleles={1, 2, 3, 4}, cap=1)),
    # k_gl<5, 2, false>: -doUnobserved 1, two to five alleles (NG 3, 6, 10, 15)
    "k_gl-A5": (dict(seed=22, depth=6.0, error_rate=0.001, do_unobserved=1, add_qs=1), (0, 8, None), (0, 1), (1, 63, 65, 130), dict(alleles={2, 3, 4, 5}, cap=1)),
    # k_gl<5, 1, false>: GL model 1 (errmod)
    "k_gl-model1": (dict(seed=23, depth=8.0, error_rate=0.01, gl_model=1, add_qs=1), (0, 4, None), (0, 1), (1, 63, 65, 130), dict()),
    # k_gl<5, 2, true>: --precise-gl 1 with per-read error probabilities
    "precise": (dict(seed=24, depth=7.0, error_rate=0.01, precise_gl=1, **BETA), (0, 8, None), (0, 1), (1, 63, 65, 130), dict(cap=1)),
    # --precise-gl 1 at --error-rate 0: a mismatching read's term is log10(0) = -inf, which stands next to the 0 of the matching genotype
    "precise-error-rate-0": (dict(seed=25, depth=4.0, error_rate=0.0, precise_gl=1, add_qs=1), (0, 8, None), (0, 1), (1, 63, 65, 130), dict(inf=1, cap=1)),
    # --error-rate 0.9: score 0, whose homT term is -inf in the table of k_gl<., 2, false>
    "k_gl-score-0": (dict(seed=26, depth=4.0, error_rate=0.9, add_qs=1), (0, 8, None), (0, 1), (65, 130), dict(inf=1, cap=1)),
    # depth 40 at --error-rate 0.001 (score 30, 3.0 per mismatching read): GL passes -37.9 ... -45.2 and goes on beyond -100; PL caps
    # (the planes context is eligible for k_gl2, gl_wpb 16, but a tile with GP stays with k_gl: vgl_launch_gl)
    "k_gl-depth40-score-30": (dict(seed=27, depth=40.0, error_rate=0.001, add_qs=1), (0, {0: 16, 1: 8}, None), (0, 1), (63, 130), dict(sub=1, cap=1)),
    # --rm-empty-sites 1 at depth 0.3: skipped sites at N = 1 and 5, readless samples everywhere
    "rm-empty-sites": (dict(seed=28, depth=0.3, error_rate=0.01, rm_empty_sites=1), (0, 4, None), (0, 1), (1, 5, 63), dict(skip=1)),
    # k_gl2<5> with every tag (hooks build, VGL_GL2X=2; planes layout only) at depth 20, score 20: 2.0 per mismatching read, GL passes
    # the subnormal range of 10^x in a tenth of the values
    "k_gl2": (dict(seed=29, depth=20.0, error_rate=0.01), (0, 16, {"VGL_GL2X": "2"}), (0,), (1, 63, 65, 130), dict(sub=1, cap=1)),
    # ... with the pool's limit at 1: every workgroup with a three-base evaluation is written again by k_gl_redo (k_gl's body)
    "k_gl_redo": (dict(seed=31, depth=20.0, error_rate=0.05), (0, 16, {"VGL_GL2X": "2", "VGL_DEBUG_GL2_OVC": "1"}), (0,), (1, 63, 65, 130), dict(sub=1, cap=1)),
    # the shipped library's own choice of k_gl2: a tile without GP (its epilogue there carries PL and pl_u8 only)
    "k_gl2-shipped": (dict(seed=32, depth=20.0, error_rate=0.01), (0, 16, None), (0,), (65, 130), dict(cap=1, no_gp=1)),
    # the fused build (N > 128, mean depth below 12, one fixed score): the plain build writes no GP -- PL and pl_u8 are checked there --,
    # the general build (GP asked for, or sample-major records) does
    "fused-plain": (dict(seed=33, depth=5.0, error_rate=0.01), (1, 8, None), (0,), (130,), dict(no_gp=1)),
    "fused-general": (dict(seed=34, depth=5.0, error_rate=0.01), (1, 8, None), (0, 1), (130,), dict(cap=1)),
}
TILE_CASES = [(name, sm, N) for name, v in PATHS.items() for sm in v[2] for N in v[3]]


def case_ids(cases):
    return [f"{n}-{'sm' if s else 'planes'}-N{N}" for n, s, N in cases]


def case_args(entry, sm):
    """the VcfglArgs of a table entry in tile mode"""
    kw, _, _, _, occur = entry
    args = VcfglArgs(add_pl=1, add_gp=0 if occur.get("no_gp") else 1, **kw)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    if sm:
        args.out_layout = _abi.VGL_LAYOUT_SAMPLE_MAJOR
    return args


def case_sites(entry, N):
    """(number of sites, true genotypes) of a table entry at N samples; occur["sites"] overrides SITES"""
    S = entry[4].get("sites", SITES[N])
    return S, M.mixed_sites(S, N, seed=1000 + N)


def case_fields(entry):
    return ["fmt_dp", "gl", "pl", "pl_u8"] + ([] if entry[4].get("no_gp") else ["gp"]) + list(entry[4].get("fields", ()))


def staging_capacity(depth):
    """the staged reads per evaluation of a context at this mean depth (mean + 8 sigma + 16, a multiple of 4: vgl_ctx_info_t.read_cap)"""
    return (int(math.ceil(depth + 8.0 * math.sqrt(depth) + 16.0)) + 3) & ~3


def open_case(entry, name, sm, N, monkeypatch):
    """the Simulator of a table entry, with the build it runs asserted from vgl_ctx_info(): (sim, args, info)"""
    from vcfgl_amd import Simulator
    kw, (fused, wpb, env), _, _, occur = entry
    args = case_args(entry, sm)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    S, _ = case_sites(entry, N)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S, hooks=env is not None)
    info = sim.info()
    if isinstance(wpb, dict):
        wpb = wpb[sm]
    want_wpb = 4 if (args.gl_model == 1 or kw["depth"] < 1.0) else wpb      # (no lane sort below a mean depth of 1: four wavefronts)
    assert (info["fused"], info["gl_wpb"], info["test_hooks"]) == (fused, want_wpb, 1 if env is not None else 0), (name, info)
    return sim, args, info


def simulate_case(name, sm, N, monkeypatch):
    entry = PATHS[name]
    sim, _, _ = open_case(entry, name, sm, N, monkeypatch)
    _, gt = case_sites(entry, N)
    t = sim.simulate(3, gt, fields=case_fields(entry))
    sim.close()
    return t, entry[4]


def canon_alleles(tile, name, sample_major):
    """a planeA field of a tile (FORMAT/AD, ADF, ADR) as [site][A][sample]; 0 where the sample-major layout holds nothing"""
    a = tile.numpy(name)
    if not sample_major:
        return a.copy()
    S, A, N = a.shape
    out = np.zeros((S, A, N), dtype=a.dtype)
    na, st = tile.numpy("n_alleles"), tile.numpy("site_status")
    for s in range(S):
        k = int(na[s]) if st[s] >= 0 else 0
        if k:
            out[s, :k, :] = a[s].reshape(-1)[: N * k].reshape(N, k).T
    return out


# ------------------------------------------------------------------------------------------------ the GL body: added cases and the check
QS_BINS = [(0, 14, 10), (15, 19, 17), (20, 24, 22), (25, 254, 30)]
AD_TAGS = dict(add_fmt_ad=1, add_fmt_adf=1, add_fmt_adr=1, add_info_dp=1, add_info_ad=1, add_info_adf=1, add_info_adr=1)
COUNT_FIELDS = ("fmt_ad", "fmt_adf", "fmt_adr", "info_dp", "info_ad", "info_adf", "info_adr", "qs", "i16")
DUMP_FIELDS = ["fmt_dp", "fmt_ad", "fmt_adf", "fmt_adr", "info_dp", "info_ad", "info_adf", "info_adr"]      # what the call with the dump is asked for besides
# the smallest shapes that reach the code (same tuple as PATHS; occur: "sites" the tile's sites, "deep" an evaluation beyond 255 reads,
# "adj" a read whose adjusted score differs from its raw one, "fields" / "counts" the read-derived tags)
BODY_EXTRA = {
    # --error-qs 1: one beta deviate per site decides the base calls; GL keeps the fixed score of --error-rate
    "error-qs-1": (dict(seed=41, depth=6.0, error_rate=0.01, error_qs=1, beta_variance=1e-5), (0, 8, None), (0,), (65,), dict()),
    # --adjust-qs 1 (the adjusted score enters GL) with --qs-bins: the dump carries the raw binned score, GL the adjusted binned one
    "adjust-qs-bins": (dict(seed=42, depth=7.0, error_rate=0.01, adjust_qs=1, adjust_by=0.499, qs_bins=QS_BINS, **BETA), (0, 8, None), (0,), (65,), dict(adj=1)),
    # -doUnobserved 0 ... 5: one to five alleles, <*> and <NON_REF>, the exploded lists
    "unobserved-0": (dict(seed=43, depth=6.0, error_rate=0.001, do_unobserved=0), (0, 8, None), (0,), (65,), dict(alleles={1, 2, 3, 4})),
    "unobserved-1": (dict(seed=44, depth=6.0, error_rate=0.001, do_unobserved=1), (0, 8, None), (0,), (65,), dict(alleles={2, 3, 4, 5})),
    "unobserved-2": (dict(seed=45, depth=6.0, error_rate=0.001, do_unobserved=2), (0, 8, None), (0,), (65,), dict(alleles={2, 3, 4, 5})),
    "unobserved-3": (dict(seed=46, depth=6.0, error_rate=0.001, do_unobserved=3), (0, 8, None), (0,), (65,), dict(alleles={4})),
    "unobserved-4": (dict(seed=47, depth=6.0, error_rate=0.001, do_unobserved=4), (0, 8, None), (0,), (65,), dict(alleles={5})),
    "unobserved-5": (dict(seed=48, depth=6.0, error_rate=0.001, do_unobserved=5), (0, 8, None), (0,), (65,), dict(alleles={5})),
    # depth 400: several pool segments per wavefront in the sampler, 400 roundings per value, every evaluation beyond 255 reads
    "depth-400": (dict(seed=50, depth=400.0, error_rate=0.01, **BETA), (0, 8, None), (0,), (5,), dict(sites=3, deep=1)),
    # the tags that are sums over the reads, with per-read scores so that the quality sums vary
    "counts": (dict(seed=51, depth=6.0, error_rate=0.01, add_qs=1, add_i16=1, **AD_TAGS, **BETA), (0, 8, None), (0, 1), (130,), dict(fields=COUNT_FIELDS, counts=1)),
}
BODY_TABLE = dict(PATHS, **BODY_EXTRA)
BODY_CASES = [(name, sm, N) for name, v in BODY_TABLE.items() for sm in v[2] for N in v[3]]


def model_flags(args):
    return dict(error_qs=args.error_qs, precise_gl=args.precise_gl, error_rate=args.error_rate, adjust_qs=args.adjust_qs, adjust_by=args.adjust_by,
                qs_bins=args.qs_bins, do_unobserved=args.do_unobserved)


def model_tile(dump, args):
    """gl_body_model.Tile of a call that asked for the dumps"""
    import gl_body_model as B
    return B.Tile(dump.numpy("reads"), dump.numpy("read_errp") if args.error_qs == 2 else None, dump.numpy("fmt_dp"), dump.numpy("alleles2acgt"),
                  dump.numpy("n_alleles"), dump.numpy("site_status"), model_flags(args))


def check_body(name, entry, args, N, sm, t, dump):
    """What a build wrote (tile `t`) against tests/gl_body_model.py on the reads of `dump` (the same call, or a second one with the same
    flags, seed, site0 and genotypes).  Asserts everything test_gpu_gl_body.py's docstring states; returns (report line, worst error /
    bound, values not identical to the replay)."""
    import gl_body_model as B
    occur = entry[4]
    for f in ("fmt_dp", "site_status", "n_alleles", "alleles2acgt"):
        assert np.array_equal(t.numpy(f), dump.numpy(f)), f"{f} differs between the call under test and the call with the dump"
    na, st, dp = t.numpy("n_alleles"), t.numpy("site_status"), t.numpy("fmt_dp")
    deepest = int(dp.max(initial=0))
    assert dump.numpy("reads").shape[0] >= deepest, "the dump is shorter than the tile's largest depth"
    mt = model_tile(dump, args)
    gl = M.canon_bits(t, "gl", sm)
    live = M.check_gl_invariants(gl, na, st, dp)
    assert np.array_equal(live, mt.live)
    n, worst, nonid = int(live.sum()), 0.0, 0
    msg = f"{name} {'sample-major' if sm else 'planes'} N={N}: {n} values, largest depth {deepest}, n_alleles {sorted(set(na[st == 0].tolist()))}"
    if args.gl_model == 2:
        x, bound, _ = B.gl2_exact(mt)
        _, worst, misplaced = B.compare_gl(gl, x, bound, live)
        replay = B.gl2_replay(mt)
        differ = gl != replay
        nonid = int(differ.sum())
        far = int((B.ulp_distance(gl[differ], replay[differ]) > 1).sum())
        msg += f", worst |GL - definition| / bound {worst:.4f}, {nonid} not identical to the float32 recurrence ({far} by more than one unit in the last place)"
        print(msg)
        assert misplaced == 0, msg
        assert worst <= 1.0, msg
        if args.precise_gl:
            assert nonid <= 1e-5 * n and far == 0, msg
        else:
            assert nonid == 0, msg
    else:
        want, tol = B.gl1_cost_differences(mt, 1.0 - args.gl1_theta)
        assert deepest <= 255
        with np.errstate(invalid="ignore"):
            got = -10.0 * gl.view(np.float32).astype(np.float64)
            ratio = np.where(live, np.abs(got - np.where(live, want, 0.0)) / np.where(live, tol, 1.0), 0.0)
        worst = float(ratio.max(initial=0.0))
        msg += f", worst |cost difference - model| / tolerance {worst:.4f}"
        print(msg)
        assert worst <= 1.0, msg
    # the counts: every field of COUNT_FIELDS that either call returned (the call under test first)
    src = {f: (t if f in t.arrays else dump) for f in COUNT_FIELDS if f in t.arrays or f in dump.arrays}
    c = B.counts_from_reads(mt, mapq=args.i16_mapq)
    got = dict(fmt_dp=dp)
    if "fmt_ad" in src:
        got["fmt_ad"] = canon_alleles(src["fmt_ad"], "fmt_ad", sm)
    if "fmt_adf" in src and "fmt_adr" in src:
        got["fmt_adfr"] = canon_alleles(src["fmt_adf"], "fmt_adf", sm) + canon_alleles(src["fmt_adr"], "fmt_adr", sm)
    if "info_adf" in src and "info_adr" in src:
        got["info_adfr"] = src["info_adf"].numpy("info_adf") + src["info_adr"].numpy("info_adr")
    for f in ("info_dp", "info_ad", "qs"):
        if f in src:
            got[f] = src[f].numpy(f)
    if "i16" in src:
        got["i16"] = src["i16"].numpy("i16")[:, :12]
    qs_worst = B.check_counts(c, got, N)
    if occur.get("counts"):
        assert set(got) == {"fmt_dp", "fmt_ad", "fmt_adfr", "info_dp", "info_ad", "info_adfr", "i16", "qs"} and all(src[f] is t for f in src)
        print(f"{name}: DP, AD, ADF + ADR, INFO/DP, INFO/AD, I16 1-12 equal the counts of {int(c['info_dp'].sum())} reads; worst QS error / bound {qs_worst:.4f}")
        assert c["i16"][:, 2].max() > 0 and (t.numpy("fmt_adf") > 0).any() and (t.numpy("fmt_adr") > 0).any()
    else:
        assert {"fmt_ad", "fmt_adfr", "info_dp", "info_ad"} <= set(got), sorted(got)
    # what the case is meant to produce
    assert n > 0
    if "alleles" in occur:
        need = occur["alleles"] if N >= 63 else set(sorted(occur["alleles"])[:2])
        assert set(na[st == 0].tolist()) >= need, msg
    if occur.get("inf"):
        assert int((gl[live] == M.F32_NEG_INF_BITS).sum()) > 0, msg      # (next to the 0 check_gl_invariants found in every evaluation)
    if occur.get("deep"):
        assert deepest > 255, msg
    if occur.get("adj"):
        act = np.arange(mt.reads.shape[0])[:, None, None] < mt.depth[None]
        assert (B.gl_scores(mt.reads, mt.read_errp, mt.flags)[act] != (mt.reads[act].astype(np.int64) >> 2)).any(), msg
    if occur.get("skip"):
        assert ((st < 0).sum() > 0) == (N <= 5), msg
    elif N >= 63:
        assert ((dp == 0) & (st == 0)[:, None]).any(), msg              # 3 % missing calls: samples without reads at written sites
    return msg, worst, nonid
