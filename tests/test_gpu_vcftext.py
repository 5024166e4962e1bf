"""The device VCF text formatter (csrc/vgl_text.hip: vgl_text_format_device, vgl_simulate_tile_text_async) against the Python model of
the host writer's text (tests/vcftext_model.py): number formatting over millions of float bit patterns and the int32 edges, whole
simulated tiles in sample-major layout, the capacity contract, and the record-loop entry (two tiles in flight, deep re-runs)."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
import vcftext_model as vm
from vcfgl_amd import Simulator, VcfglArgs, _abi, vcftext

pytestmark = pytest.mark.gpu
TAGS = [("DP", "fmt_dp", "add_fmt_dp"), ("GL", "gl", "add_gl"), ("PL", "pl", "add_pl"), ("GP", "gp", "add_gp"), ("AD", "fmt_ad", "add_fmt_ad"),
        ("ADF", "fmt_adf", "add_fmt_adf"), ("ADR", "fmt_adr", "add_fmt_adr")]


def one_value_columns(values, is_float, N=1000):
    """device text of `values` laid out as sites of N one-valued samples, and the tokens read back from it"""
    n = len(values)
    S = (n + N - 1) // N
    a = np.zeros(S * N, dtype=np.uint32 if is_float else np.int32)
    a[:n] = values
    t = torch.from_numpy(a.view(np.float32 if is_float else np.int32).reshape(S, N)).cuda()
    st = torch.zeros(S, dtype=torch.int32, device="cuda")
    na = torch.full((S,), 2, dtype=torch.int32, device="cuda")
    text, off = vcftext.format_columns([("X", t, vcftext.ONE)], st, na, N)
    lines = bytes(text.cpu().numpy()).decode().split("\n")
    assert lines[-1] == "" and len(lines) == S + 1
    toks = []
    for ln in lines[:-1]:
        f = ln.split("\t")
        assert f[0] == "" and f[1] == "X" and len(f) == N + 2
        toks += f[2:]
    return toks[:n]


def test_float_sweep_equals_the_model():
    """the class boundaries of the formatter, random patterns, and every 8th float of whole binades around 1e-4, 1 and 1e6"""
    pats = [vm.float_corpus(n_random=400000, seed=3)]
    for lo in (0x38800000, 0x3F800000, 0x49000000):                          # [2^-14, 2^-13) (holds 1e-4), [1, 2), [2^19, 2^20)
        pats.append(np.arange(lo, lo + 0x800000, 8, dtype=np.uint32))
    pats.append(np.arange(0x49742400 - 200000, 0x49742400 + 200000, dtype=np.uint32))          # around 1e6, every float
    pats = np.unique(np.concatenate(pats))
    assert len(pats) > 4_000_000
    got = one_value_columns(pats, True)
    want = [vm.fmt_float_bits(p) for p in pats]
    bad = [(hex(int(p)), g, w) for p, g, w in zip(pats, got, want) if g != w]
    assert not bad, (len(bad), bad[:20])


def test_int32_edges():
    vals = np.array([vm.INT32_MISSING, vm.INT32_MISSING + 1, -1000000000, -999999999, -10, -9, -1, 0, 1, 9, 10, 99, 100, 999999999,
                     1000000000, 2 ** 31 - 1] + list(range(-1500, 1500)), dtype=np.int64).astype(np.int32)
    assert one_value_columns(vals, False, N=7) == [vm.fmt_int(v) for v in vals]


def simulate_tile(args, N, S, site0=0, seed=1, hooks=False):
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    args.out_layout = _abi.VGL_LAYOUT_SAMPLE_MAJOR
    sim = Simulator(args, N, max_sites_per_tile=S, hooks=hooks)
    fields = ["site_status", "n_alleles"] + [name for _, name, flag in TAGS if getattr(args, flag)]
    tile = sim.new_tile(S, fields=fields, device="cuda:0")
    gt = synth.acgt_sites(S, N, seed=seed, missing=0.03)
    sim.simulate_device(site0, torch.from_numpy(gt).cuda(), tile)
    sim.check()
    torch.cuda.synchronize()
    return sim, tile, gt


def model_text(args, tile, N):
    fields = [(key, tile.numpy(name).reshape(tile.n_sites, -1), kind) for key, name, _, kind, flag in vcftext.FORMAT_ORDER if getattr(args, flag)]
    return vm.render(fields, tile.numpy("site_status"), tile.numpy("n_alleles"), N)


def check_tile(args, N, S, **kw):
    sim, tile, _ = simulate_tile(args, N, S, **kw)
    text, off = vcftext.format_columns(vcftext.tile_fields(args, tile), tile["site_status"], tile["n_alleles"], N)
    want, woff = model_text(args, tile, N)
    sim.close()
    assert np.array_equal(off.cpu().numpy(), woff)
    got = bytes(text.cpu().numpy())
    assert got == want
    return tile, got


@pytest.mark.parametrize("tag", [t[0] for t in TAGS] + ["all", "none"])
def test_each_tag_alone_and_all_together(tag):
    flags = {flag: int(tag == "all" or key == tag) for key, _, flag in TAGS}
    args = VcfglArgs(seed=11, depth=4, error_rate=0.02, do_unobserved=1, **flags)
    check_tile(args, 7, 67)


@pytest.mark.parametrize("du,N,S,kw", [(0, 1, 65, {}), (1, 7, 300, {}), (2, 1000, 33, {}), (3, 2500, 6, {}), (4, 7, 257, {}), (5, 1000, 19, {}),
                                       (1, 3, 200, dict(rm_empty_sites=1, depth=0.3)), (2, 1000, 17, dict(error_qs=2, beta_variance=1e-4)),
                                       (1, 60, 99, dict(gl_model=1)), (1, 65, 70, dict(precise_gl=1, error_qs=1, beta_variance=1e-5))])
def test_whole_tiles_equal_the_model(du, N, S, kw):
    """-doUnobserved 0..5 (nA 1..5, G = 10 and 15), skipped sites (--rm-empty-sites 1 at a low depth), N in {1, 3, 7, 60, 65, 1000, 2500}, tile
    sizes that are not multiples of a workgroup, every tag"""
    base = dict(seed=5 + du, depth=6, error_rate=0.01, do_unobserved=du)
    base.update(kw)
    args = VcfglArgs(add_gl=1, add_pl=1, add_gp=1, add_fmt_dp=1, add_fmt_ad=1, add_fmt_adf=1, add_fmt_adr=1, **base)
    tile, _ = check_tile(args, N, S)
    st = tile.numpy("site_status")
    if kw.get("rm_empty_sites"):
        assert (st < 0).any() and (st >= 0).any()


def test_capacity_one_byte_short_writes_nothing():
    args = VcfglArgs(seed=3, depth=5, error_rate=0.01, add_pl=1, add_gp=1)
    sim, tile, _ = simulate_tile(args, 100, 50)
    fields = vcftext.tile_fields(args, tile)
    text, off = vcftext.format_columns(fields, tile["site_status"], tile["n_alleles"], 100)
    total = int(off[-1])
    assert total == text.numel() > 0
    dst = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    o2 = vcftext.format_into(fields, tile["site_status"], tile["n_alleles"], 100, dst, dst_cap=total - 1)
    torch.cuda.synchronize()
    assert int(o2[-1]) == total                                    # the size it needs is reported
    assert bool((dst == 0xA5).all())                               # nothing written
    o3 = vcftext.format_into(fields, tile["site_status"], tile["n_alleles"], 100, dst, dst_cap=total)
    torch.cuda.synchronize()
    assert torch.equal(o3, off) and torch.equal(dst[:total], text) and bool((dst[total:] == 0xA5).all())
    lib = _abi.load_library()
    bad = (_abi.TextField * 1)(_abi.TextField(b"X", 0, 7, tile["gl"].data_ptr(), 1))
    assert lib.vgl_text_format_device(0, bad, 1, 100, 50, tile["site_status"].data_ptr(), tile["n_alleles"].data_ptr(), dst.data_ptr(),
                                      dst.numel(), o3.data_ptr(), None, 0, None) == _abi.VGL_E_ARG
    sim.close()


def ctx_text(sim, site0, gts, text_cap=None):
    """vgl_simulate_tile_text_async for consecutive tiles, all in flight before the first wait: [(text, offsets, tile)]"""
    lib = sim.lib
    cap = int(lib.vgl_ctx_text_bound(sim.ctx, sim.max_sites_per_tile))
    subs = []
    for k, gt in enumerate(gts):
        tile = sim.new_tile(gt.shape[0], fields=["fmt_dp"])
        buf = np.full(cap, 0x5A, dtype=np.uint8)
        off = np.zeros(gt.shape[0] + 1, dtype=np.int64)
        t = C.c_int32()
        gt = np.ascontiguousarray(gt)
        sim._check(lib.vgl_simulate_tile_text_async(sim.ctx, site0 + sum(g.shape[0] for g in gts[:k]), gt.shape[0], gt.ctypes.data, tile.byref(),
                                                     buf.ctypes.data, cap if text_cap is None else text_cap, off.ctypes.data, C.byref(t)))
        subs.append((t.value, buf, off, tile, gt))
    out = []
    for t, buf, off, tile, gt in subs:
        rc = lib.vgl_tile_wait(sim.ctx, t)
        out.append((rc, buf, off, tile))
    return out


ALL = dict(add_gl=1, add_pl=1, add_gp=1, add_fmt_ad=1, add_fmt_adf=1, add_fmt_adr=1)


def test_record_loop_entry_equals_the_stateless_entry():
    """two tiles in flight through vgl_simulate_tile_text_async / vgl_tile_wait give the bytes of vgl_text_format_device on the same tiles"""
    N, S = 300, 64

    def mk():
        return VcfglArgs(seed=21, depth=5, error_rate=0.01, do_unobserved=2, **ALL)
    sim, _, _ = simulate_tile(mk(), N, S)                              # sample-major contexts (their first tiles are not used)
    ref, _, _ = simulate_tile(mk(), N, S)
    gts = [synth.acgt_sites(S, N, seed=40 + k, missing=0.03) for k in range(2)]
    res = ctx_text(sim, 100, gts)
    fields = ["site_status", "n_alleles"] + [name for _, name, flag in TAGS if getattr(ref.args, flag)]
    for k, ((rc, buf, off, tile), gt) in enumerate(zip(res, gts)):
        assert rc == _abi.VGL_OK, sim.lib.vgl_last_error()
        dtile = ref.new_tile(S, fields=fields, device="cuda:0")
        ref.simulate_device(100 + k * S, torch.from_numpy(gt).cuda(), dtile)
        ref.check()
        want, woff = vcftext.format_columns(vcftext.tile_fields(ref.args, dtile), dtile["site_status"], dtile["n_alleles"], N)
        assert np.array_equal(off, woff.cpu().numpy())
        total = int(off[-1])
        assert bytes(buf[:total]) == bytes(want.cpu().numpy())
        assert (buf[total:] == 0x5A).all()                          # only the tile's bytes were copied
        for f in ("site_status", "n_alleles", "fmt_dp"):
            assert np.array_equal(tile.numpy(f), dtile.numpy(f)), f
    # a text larger than text_cap: VGL_E_CAPACITY, the size needed, nothing written
    rc, buf, off, _ = ctx_text(sim, 100, gts[:1], text_cap=1000)[0]
    assert rc == _abi.VGL_E_CAPACITY and int(off[-1]) > 1000 and (buf == 0x5A).all()
    sim.close()
    ref.close()


def test_layout_planes_context_is_refused():
    args = VcfglArgs(seed=1, depth=3, error_rate=0.01)
    sim = Simulator(args, 10, max_sites_per_tile=4)
    tile = sim.new_tile(4, fields=["fmt_dp"])
    gt = synth.acgt_sites(4, 10, seed=1)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    off = np.zeros(5, dtype=np.int64)
    t = C.c_int32()
    assert sim.lib.vgl_simulate_tile_text_async(sim.ctx, 0, 4, gt.ctypes.data, tile.byref(), buf.ctypes.data, buf.size, off.ctypes.data, C.byref(t)) == _abi.VGL_E_ARG
    sim.close()


def test_deep_rerun_gives_the_same_text(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (hooks build): every tile draws deeper than the staging capacity and vgl_tile_wait runs it again through the
    sibling context into device planes, formats and copies again -- the text equals the text without the hook"""
    N, S = 100, 40
    gts = [synth.acgt_sites(S, N, seed=70 + k, missing=0.03) for k in range(2)]

    def run(hooks):
        args = VcfglArgs(seed=42, depth=20, error_rate=0.01, add_pl=1, add_fmt_ad=1)
        args.rng_mode, args.beta_sampler, args.out_layout = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48, _abi.VGL_LAYOUT_SAMPLE_MAJOR
        sim = Simulator(args, N, max_sites_per_tile=S, hooks=hooks)
        if hooks:
            assert sim.info()["read_cap"] == 8
        r = ctx_text(sim, 3, gts)
        sim.close()
        return r

    plain = run(False)
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    deep = run(True)
    for (rc0, b0, o0, t0), (rc1, b1, o1, t1) in zip(plain, deep):
        assert rc0 == rc1 == _abi.VGL_OK
        assert np.array_equal(o0, o1) and bytes(b0[:o0[-1]]) == bytes(b1[:o1[-1]])
        assert np.array_equal(t0.numpy("fmt_dp"), t1.numpy("fmt_dp"))
        assert int(t1.numpy("fmt_dp").max()) > 8
