"""vgl_params.layout is public ABI: a caller may pass its own block, off[4] and qs_read_stride (include/vcfgl_hip.h, vgl_rng_layout).
The library derives from it k_sitebase's power table, the per-sample jump table, qs_read_tab (J^(stride r)), the 52-bit split
stepping of k_sample<0>, k_redo, k_tail and the sibling context of the deep re-run (vcfgl_amd/csrc/hostlib/plan.h, "rand48 addressing", and the jump tables of hostlib/tables.h); every other
test runs these at the default layout only -- one stride (32) and one family of blocks.  Here every build that reads the layout in
code of its own runs under caller layouts and must equal the oracle bit for bit (test_gpu_parity.assert_parity), at a small site0
and within the last 100 sites the layout can address (vgl_rng_tile_max_sites).

Layouts (d = ceil of the largest mean depth, s1 = 4 d + 64 the haplotype sub-window):
  default     the library's own (control)
  tight       qs_read_stride 5, block = the smallest odd value >= 64 + s1 (4 + 5)
  even        block = the smallest power of two >= the default block (an even block)
  huge        block = 2^33 + 1, N <= 3: exponents near 2^48, 64-bit products in k_sitebase and the sample table
  permuted    the default sub-windows in the order off[3] < off[0] < off[2] < off[1]
  stride1 / stride7 / stride4096   qs_read_stride (the block grown for 4096)
  shared      off = (0, 0, 0, 0): legal ("only statistically overlapping"); parity must still hold"""
import ctypes as C

import numpy as np
import pytest

import synth
from test_gpu_parity import STRAND, assert_parity
from test_rng_windows_cpu import site_hash
from vcfgl_amd import Simulator, VcfglArgs, VglError, _abi

gpu = pytest.mark.gpu

BETA = dict(error_qs=2, beta_variance=1e-5)
# name -> (flags, N, what vgl_ctx_info must report, environment of the hooks build)
BUILDS = {
    "eq0-depth5-N300-fused": (dict(depth=5.0), 300, dict(fused=1), None),
    "eq0-depth20-three-kernels": (dict(depth=20.0, add_pl=1, add_fmt_ad=1), 65, dict(fused=0, depth_mode=_abi.VGL_DEPTH_KDEPTH), None),
    "eq2-default-tags-split-redo": (dict(depth=20.0, **BETA), 300, dict(sample_lean=2), None),
    "eq2-addQS-addI16-strand-lean3": (dict(depth=20.0, add_qs=1, **BETA, **STRAND), 65, dict(sample_lean=3), None),
    "eq2-precise-gl": (dict(depth=20.0, precise_gl=1, add_pl=1, **BETA), 65, {}, None),
    "eq1": (dict(depth=7.0, error_qs=1, beta_variance=1e-4, add_fmt_ad=1), 1, {}, None),
    "GL1": (dict(depth=9.0, gl_model=1, add_pl=1), 65, {}, None),
    "per-sample-depths-kdepth": (dict(depths=True, add_fmt_ad=1), 300, dict(depth_mode=_abi.VGL_DEPTH_KDEPTH), None),
    "eq2-addI16-deep-rerun-readcap8": (dict(depth=20.0, add_i16=1, add_fmt_adf=1, **BETA), 65, dict(read_cap=8), {"VGL_DEBUG_READ_CAP": "8"}),
}
LAYOUTS = ["default", "tight", "even", "huge", "permuted", "stride1", "stride7", "stride4096", "shared"]
CASES = [(b, l) for b in BUILDS for l in LAYOUTS if not (l == "huge" and "fused" in b)]     # (the fused kernel needs N > 128; huge only with N <= 3)


def make_args(build, N):
    kw = dict(BUILDS[build][0])
    if kw.pop("depths", False):
        kw["depths"] = [12.0 + (s % 7) for s in range(N)]
    a = VcfglArgs(seed=42, error_rate=kw.pop("error_rate", 0.01), **kw)
    a.rng_mode, a.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    return a


def make_layout(name, args, N):
    """the rng_layout of the table above for these flags (None: the library's default)"""
    p, _keep = args.to_struct(N)
    lay = _abi.RngLayout()
    assert _abi.load_library().vgl_default_rng_layout(C.byref(p), C.byref(lay)) == 0
    block, off, stride = int(lay.block), [int(lay.off[k]) for k in range(4)], int(lay.qs_read_stride)
    d = int(np.ceil(max(args.depths) if args.depths is not None else args.depth))
    s0, s1 = 64, 4 * d + 64
    assert off == [0, s0, s0 + s1, s0 + 4 * s1] and stride == 32
    s3 = block - off[3]
    if name == "default":
        return None
    if name == "tight":
        return ((s0 + s1 * (4 + 5)) | 1, off, 5)
    if name == "even":
        return (1 << (block - 1).bit_length(), off, stride)
    if name == "huge":
        return ((1 << 33) + 1, off, stride)
    if name == "permuted":
        perm = [s3, s3 + s0 + 3 * s1, s3 + s0, 0]
        assert perm[3] < perm[0] < perm[2] < perm[1] and perm[1] + s1 <= block
        return (block, perm, stride)
    if name == "shared":
        return (block, [0, 0, 0, 0], stride)
    stride = int(name[len("stride"):])
    return (max(block, (s0 + 4 * s1 + stride * s1) | 1), off, stride)


def max_sites(args, N):
    p, _keep = args.to_struct(N)
    mx = C.c_int64()
    assert _abi.load_library().vgl_rng_tile_max_sites(C.byref(p), C.byref(mx)) == 0
    return mx.value


@gpu
@pytest.mark.parametrize("build,layout", CASES, ids=[f"{b}-{l}" for b, l in CASES])
def test_caller_layout_equals_the_oracle(oracle, monkeypatch, build, layout):
    _, N, want_info, env = BUILDS[build]
    if layout == "huge":
        N = min(N, 3)
        want_info = {k: v for k, v in want_info.items() if k != "sample_lean"}      # (which k_sample a shape of three samples gets is not the point)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    args = make_args(build, N)
    args.rng_layout = make_layout(layout, args, N)
    S = 24 if N <= 65 else 9
    mx = max_sites(args, N)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S, hooks=env is not None)
    info = sim.info()
    assert info["rng_tile_max_sites"] == mx
    for k, v in want_info.items():
        assert info[k] == v, (k, info[k])
    o = oracle.Oracle(args, N)
    for site0 in (5, mx - S - 3):                                   # ... and within the last 100 sites of the layout
        assert site0 == 5 or mx - 100 <= site0 and site0 + S <= mx
        gt = synth.acgt_sites(S, N, seed=S + N, missing=0.03)
        got = sim.simulate(site0, gt)
        want = o.simulate(site0, gt, fields=sim.default_fields())
        if env:
            assert int(want.numpy("fmt_dp").max()) > 8             # the tile was run again on the sibling context
        assert_parity(want, got, exact_gl=not args.precise_gl, i16=True, check_gp=False)
    sim.close()


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l != "default"])
def test_max_sites_and_site_hash_under_a_caller_layout(layout):
    """pure host arithmetic: the largest power of two with 2^W n_samples block <= 2^48, and H of include/vcfgl_hip.h on [0, 2^W)"""
    lib = _abi.load_library()
    for build, N in (("eq2-default-tags-split-redo", 300), ("eq0-depth5-N300-fused", 3), ("eq1", 1)):
        args = make_args(build, N)
        args.rng_layout = make_layout(layout, args, N)
        p, _keep = args.to_struct(N)
        mx = max_sites(args, N)
        W = mx.bit_length() - 1
        assert mx == 1 << W and (mx * N * args.rng_layout[0] <= 1 << 48 < 2 * mx * N * args.rng_layout[0] or W == 40)
        h = C.c_int64()
        rnd = np.random.default_rng(W)
        for site in [0, 1, 2, mx - 1] + [int(x) for x in rnd.integers(0, mx, 300)]:
            assert lib.vgl_rng_tile_site_hash(C.byref(p), site, C.byref(h)) == 0
            assert h.value == site_hash(site, W)
        assert lib.vgl_rng_tile_site_hash(C.byref(p), mx, C.byref(h)) == _abi.VGL_E_ARG


@gpu
def test_a_zero_read_stride_is_refused_with_per_read_scores():
    args = make_args("eq2-default-tags-split-redo", 65)
    block, off, _ = make_layout("tight", args, 65)
    args.rng_layout = (block, off, 0)
    with pytest.raises(VglError) as e:
        Simulator(args, 65, device=0, max_sites_per_tile=4)
    assert e.value.code == _abi.VGL_E_ARG and "qs_read_stride" in str(e.value)
    args = make_args("eq0-depth20-three-kernels", 65)             # without per-read scores the stride is not read
    args.rng_layout = (block, off, 0)
    Simulator(args, 65, device=0, max_sites_per_tile=4).close()


@gpu
def test_a_block_below_the_staging_capacity_is_refused_with_i16():
    """-addI16: the tail distances of an evaluation come from its window of the second sequence, one draw per staged read"""
    args = make_args("eq2-addQS-addI16-strand-lean3", 65)
    sim = Simulator(args, 65, device=0, max_sites_per_tile=4)
    cap = sim.info()["read_cap"]
    sim.close()
    _, off, stride = make_layout("tight", args, 65)
    args.rng_layout = (cap - 1, off, stride)
    with pytest.raises(VglError) as e:
        Simulator(args, 65, device=0, max_sites_per_tile=4)
    assert e.value.code == _abi.VGL_E_ARG and "staging capacity" in str(e.value)
    args.rng_layout = (cap, off, stride)                          # a window that just holds the staged reads is accepted
    Simulator(args, 65, device=0, max_sites_per_tile=4).close()
    args.add_i16 = 0
    args.rng_layout = (cap - 1, off, stride)                      # ... and without -addI16 the block is the caller's business
    Simulator(args, 65, device=0, max_sites_per_tile=4).close()
