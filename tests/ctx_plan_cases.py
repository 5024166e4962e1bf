"""The parameter sets that flip each branch of the launch plan a context derives (vcfgl_amd/csrc/hostlib/plan.h), shared by
tools/ctx_info_matrix.py (which recorded tests/golden/ctx_plan/parent_info.json), tests/test_gpu_ctx_plan.py and
tests/test_plan_core_cpu.py.

A case is a dict: `name`; `n` samples; `args`, keywords of VcfglArgs on top of BASE; optionally `max_sites` (64 unless given),
`tile` (vgl_ctx_info is recorded again after one synchronous 8-site host tile with every tag the context can produce), `raw`
(fields of the vgl_params struct overwritten after VcfglArgs.to_struct: what no VcfglArgs can express) and `null` (a null
vgl_params pointer).  A case the library refuses records the code and the text of vgl_last_error() instead."""
import ctypes as C

from vcfgl_amd import VcfglArgs, _abi

MAX_SITES = 64
TILE_SITES = 8
BASE = dict(seed=42, depth=20.0, error_rate=0.01)
# vgl_ctx_info_t fields that cannot differ between two contexts of one library on one device's build
CONSTANT_FIELDS = ("size", "abi_version", "test_hooks")
# ... and the ones the plan does not decide (tests/plan_core_main.cpp prints every other field)
NOT_PLAN_FIELDS = ("device", "workspace_bytes", "test_hooks")

_EQ2 = dict(error_qs=2, beta_variance=1e-5)                      # beta shapes 9.89 and 979: both >= 8
_BINS = [(0, 19, 10), (20, 39, 30), (40, 63, 50)]
_SERIAL = dict(rng_mode=_abi.VGL_RNG_SERIAL)

CASES = [
    # depth mode
    dict(name="depth1", n=8, args=dict(depth=1.0)),
    dict(name="depth20", n=8, args=dict(), tile=True),
    dict(name="depth250", n=8, args=dict(depth=250.0)),
    dict(name="depth_below_1", n=8, args=dict(depth=0.5)),
    dict(name="depths_5_20", n=2, args=dict(depth=None, depths=[5.0, 20.0])),
    dict(name="serial", n=8, args=dict(**_SERIAL), tile=True),
    # fused k_gl: off at N = 128, one workgroup per site, two, off above four
    dict(name="fused_n128", n=128, args=dict(depth=5.0)),
    dict(name="fused_n130", n=130, args=dict(depth=5.0)),
    dict(name="fused_n600", n=600, args=dict(depth=5.0)),
    dict(name="fused_n2100", n=2100, args=dict(depth=5.0)),
    # sample build
    dict(name="eq2_defer_lean", n=64, args=dict(**_EQ2), tile=True),
    dict(name="eq2_defer_qs", n=64, args=dict(add_qs=1, **_EQ2)),
    dict(name="eq2_small_shape", n=64, args=dict(error_qs=2, beta_variance=1e-4)),
    dict(name="eq2_small_shape_qs", n=64, args=dict(error_qs=2, beta_variance=1e-4, add_qs=1)),
    # pool
    dict(name="pool_depth1", n=64, args=dict(depth=1.0, **_EQ2)),
    dict(name="pool_depth30", n=64, args=dict(depth=30.0, **_EQ2)),
    dict(name="pool_bins", n=64, args=dict(qs_bins=_BINS, **_EQ2)),
    dict(name="pool_bins_depth30", n=64, args=dict(depth=30.0, qs_bins=_BINS, **_EQ2)),
    dict(name="pool_precise", n=64, args=dict(precise_gl=1, **_EQ2)),
    dict(name="pool_bins_above_254", n=64, args=dict(qs_bins=[(0, 19, 10), (20, 39, 30), (40, 255, 50)], **_EQ2)),
    dict(name="eq1", n=8, args=dict(error_qs=1, beta_variance=1e-5)),
    # GL build
    dict(name="gl1", n=8, args=dict(gl_model=1)),
    dict(name="gl1_deep", n=8, args=dict(gl_model=1, depth=250.0)),
    dict(name="gl1_eq2", n=8, args=dict(gl_model=1, **_EQ2)),
    dict(name="gl_rate_005", n=8, args=dict(error_rate=0.05)),
    dict(name="gl_sample_major", n=8, args=dict(out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR, add_pl=1), tile=True),
    dict(name="gl_precise", n=8, args=dict(precise_gl=1)),
    # site hash
    dict(name="hash_n3", n=3, args=dict()),
    dict(name="hash_n1000", n=1000, args=dict()),
    # other
    dict(name="i16", n=8, args=dict(add_i16=1, add_qs=1), tile=True),
    dict(name="strand", n=8, args=dict(add_fmt_adf=1, add_fmt_adr=1)),
    dict(name="no_unobserved", n=8, args=dict(do_unobserved=0)),
    dict(name="max_sites_48", n=8, args=dict(), max_sites=48),
    dict(name="serial_i16", n=8, args=dict(add_i16=1, **_SERIAL)),
    dict(name="serial_gl1_deep", n=4, args=dict(gl_model=1, depth=250.0, **_SERIAL)),
    dict(name="serial_beta_chain", n=8, args=dict(beta_sampler=_abi.VGL_BETA_STD, **_SERIAL, **_EQ2), tile=True),
    dict(name="serial_eq2_rand48", n=8, args=dict(**_SERIAL, **_EQ2)),
    # one refusal of each kind
    dict(name="refuse_null", n=8, args=dict(), null=True),
    dict(name="refuse_abi", n=8, args=dict(), raw=dict(abi_version=_abi.ABI_VERSION - 1)),
    dict(name="refuse_n_samples", n=8, args=dict(), raw=dict(n_samples=0)),
    dict(name="refuse_max_sites", n=8, args=dict(), max_sites=0),
    dict(name="refuse_gl_model", n=8, args=dict(gl_model=3)),
    dict(name="refuse_error_qs", n=8, args=dict(error_qs=3)),
    dict(name="refuse_unobserved", n=8, args=dict(do_unobserved=6)),
    dict(name="refuse_error_rate", n=8, args=dict(error_rate=1.0)),
    dict(name="refuse_n_bins", n=8, args=dict(), raw=dict(n_qs_bins=1000)),
    dict(name="refuse_bins_null", n=8, args=dict(), raw=dict(n_qs_bins=2)),
    dict(name="refuse_bin_score", n=8, args=dict(qs_bins=[(0, 39, 10), (40, 255, 70)])),
    dict(name="refuse_gl1_precise", n=8, args=dict(gl_model=1, precise_gl=1)),
    dict(name="refuse_rng_mode", n=8, args=dict(rng_mode=2)),
    dict(name="refuse_out_layout", n=8, args=dict(out_layout=2)),
    dict(name="refuse_mt_tile", n=8, args=dict(beta_sampler=_abi.VGL_BETA_STD, **_EQ2)),
    dict(name="refuse_depths", n=2, args=dict(depth=None, depths=[5.0, -1.0])),
    dict(name="refuse_depth", n=8, args=dict(depth=-1.0)),
    dict(name="refuse_read_cap", n=8, args=dict(depth=900.0)),
    dict(name="refuse_bin_range", n=8, args=dict(qs_bins=[(0, 10, 10)])),
    dict(name="refuse_adjq", n=8, args=dict(adjust_qs=3, adjust_by=-30.0, add_qs=1)),
    dict(name="refuse_beta_args", n=8, args=dict(error_qs=2, beta_variance=-1.0)),
    dict(name="refuse_beta_shape", n=8, args=dict(error_qs=2, beta_variance=0.1)),
    dict(name="refuse_period", n=3, args=dict(rng_layout=(1 << 47, (0, 64, 208, 640), 32))),
    dict(name="refuse_i16_block", n=8, args=dict(add_i16=1, rng_layout=(9, (0, 1, 2, 3), 1))),
    dict(name="refuse_qs_stride", n=8, args=dict(rng_layout=(1 << 20, (0, 64, 208, 640), 0), **_EQ2)),
]


def case_args(case):
    kw = dict(BASE)
    kw.update(case["args"])
    return VcfglArgs(**kw)


def case_params(case):
    """(vgl_params or None, keepalive, max_sites) of a case"""
    if case.get("null"):
        return None, [], case.get("max_sites", MAX_SITES)
    p, keep = case_args(case).to_struct(case["n"])
    for k, v in case.get("raw", {}).items():
        setattr(p, k, v)
    return p, keep, case.get("max_sites", MAX_SITES)


def case_line(case):
    """the case as one line of `key=value` words for tests/plan_core_main.cpp: every scalar field of vgl_params, then the arrays"""
    p, keep, max_sites = case_params(case)
    words = [case["name"], f"max_sites={max_sites}"]
    if p is None:
        return " ".join(words + ["null=1"])
    for f, t in _abi.Params._fields_:
        if f in ("depths", "qs_bins", "layout"):
            continue
        v = getattr(p, f)
        words.append(f"{f}={v!r}" if isinstance(v, float) else f"{f}={v}")
    if p.depths:
        words.append("depths=" + ",".join(repr(p.depths[i]) for i in range(case["n"])))
    if p.qs_bins:
        words.append("qs_bins=" + ",".join(str(p.qs_bins[i]) for i in range(3 * p.n_qs_bins)))
    lay = p.layout
    words.append("layout=" + ",".join(str(v) for v in [lay.block, *lay.off, lay.qs_read_stride]))
    return " ".join(words)


def _info(lib, ctx):
    ci = _abi.CtxInfo()
    ci.size = C.sizeof(_abi.CtxInfo)
    assert lib.vgl_ctx_info(ctx, C.byref(ci)) == _abi.VGL_OK, lib.vgl_last_error().decode()
    return {f: getattr(ci, f) for f, _ in _abi.CtxInfo._fields_ if f != "device"}


def collect(lib, device=0):
    """{case name: {"info": ..., "info_after_tile": ...} or {"code": ..., "error": ...}} from a library on a GPU"""
    import synth
    from vcfgl_amd.tile import Tile
    out = {}
    for case in CASES:
        p, keep, max_sites = case_params(case)
        ctx = C.c_void_p()
        rc = lib.vgl_ctx_create(C.byref(p) if p is not None else None, device, max_sites, C.byref(ctx))
        if rc != _abi.VGL_OK:
            out[case["name"]] = {"code": rc, "error": lib.vgl_last_error().decode()}
            continue
        rec = {"info": _info(lib, ctx)}
        if case.get("tile"):
            args, n = case_args(case), case["n"]
            skip = {"pl_u8"} | (set() if (args.add_qs or args.add_i16) else {"qs"}) | (set() if args.add_i16 else {"i16"})
            tile = Tile(TILE_SITES, n, lib.vgl_max_alleles(C.byref(p)), lib.vgl_max_genotypes(C.byref(p)),
                        fields=[f for f, _, _ in _abi.TILE_FIELDS if f not in skip])
            gt = synth.binary_sites(0, TILE_SITES, n)
            rc = lib.vgl_simulate_tile(ctx, 0, TILE_SITES, gt.ctypes.data, tile.byref())
            assert rc == _abi.VGL_OK, (case["name"], lib.vgl_last_error().decode())
            rec["info_after_tile"] = _info(lib, ctx)
        lib.vgl_ctx_destroy(ctx)
        out[case["name"]] = rec
    return out
