"""The fetch-GL side channel of a context (vgl_ctx_fetchgl, vgl_ctx_fetchgl_next; Simulator.fetch_gl): through each of the three
asynchronous entry points the tile's fetched text equals the model (tests/fetchgl_model.py) applied to the GL that a plain run of the
same tile returns -- whether or not the caller asks for GL, in both layouts and RNG modes, with two tiles in flight, beside a
discordance tally and a pileup request, and after a tile was run again on the sibling context.  vgl_simulate_tile_device has no side
channel: its device arrays go to vgl_fetchgl_format_device."""
import ctypes as C

import numpy as np
import pytest
import torch

import fetchgl_model as fm
import synth
from vcfgl_amd import Simulator, VcfglArgs, _abi, fetchgl, recordloop

pytestmark = pytest.mark.gpu


def sim_args(mode=_abi.VGL_RNG_TILE, layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR, **kw):
    base = dict(seed=11, depth=3, error_rate=0.05, add_fmt_dp=1, add_pl=1, out_layout=layout)
    base.update(kw)
    a = VcfglArgs(**base)
    a.rng_mode = mode
    a.beta_sampler = _abi.VGL_BETA_STD if mode == _abi.VGL_RNG_SERIAL else _abi.VGL_BETA_RAND48
    return a


def model_of(args, N, site0, gt, a, b, mode, hooks=False):
    """the model applied to the GL a plain run of the tile returns (tile mode: a value depends on (seed, site, sample) alone)"""
    sim = Simulator(args, N, device=0, max_sites_per_tile=gt.shape[0], hooks=hooks)
    t = sim.simulate(site0, gt)
    G = sim.G
    sim.close()
    return fm.render(t.numpy("site_status"), t.numpy("n_alleles"), t.numpy("alleles2acgt"), np.ascontiguousarray(t.numpy("gl")).view(np.uint32).reshape(-1),
                     args.out_layout, G, a, b, mode), t


def side_channel(args, N, S, gts, entry, a, b, mode, fields, also_pileup=False):
    """vgl_ctx_fetchgl_next + one of the three async entries for consecutive tiles, two in flight"""
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    lib = sim.lib
    sim.fetch_gl(a, b, mode)
    cap = int(lib.vgl_ctx_fetchgl_bound(sim.ctx, S))
    assert cap == fetchgl.bound(N, S)
    subs, out = [], []

    def wait(t, keep):
        rc = lib.vgl_tile_wait(sim.ctx, t)
        assert rc == _abi.VGL_OK, lib.vgl_last_error()
        out.append(keep)
    for k, gt in enumerate(gts):
        if k >= 2:
            wait(*subs[k - 2])
        n = gt.shape[0]
        keep = {"text": np.full(cap, 0x5A, np.uint8), "off": np.zeros(n + 1, np.int64), "gt": np.ascontiguousarray(gt)}
        p = _abi.FetchGlTile(keep["text"].ctypes.data, cap, keep["off"].ctypes.data, -7)
        keep["p"] = p
        tile = sim.new_tile(n, fields=fields)
        keep["tile"] = tile
        sim._check(lib.vgl_ctx_fetchgl_next(sim.ctx, C.byref(p)))
        if also_pileup:
            pcap = int(lib.vgl_ctx_pileup_bound(sim.ctx, S))
            keep["ptext"], keep["poff"] = np.zeros(pcap, np.uint8), np.zeros(n + 1, np.int64)
            keep["pp"] = _abi.PileupTile(keep["ptext"].ctypes.data, pcap, keep["poff"].ctypes.data, -7)
            sim._check(lib.vgl_ctx_pileup_next(sim.ctx, C.byref(keep["pp"])))
        t = C.c_int32()
        site0 = sum(g.shape[0] for g in gts[:k])
        if entry == "plain":
            rc = lib.vgl_simulate_tile_async(sim.ctx, site0, n, keep["gt"].ctypes.data, tile.byref(), C.byref(t))
        elif entry == "text":
            tcap = int(lib.vgl_ctx_text_bound(sim.ctx, S))
            keep["vt"], keep["vo"] = np.zeros(tcap, np.uint8), np.zeros(n + 1, np.int64)
            rc = lib.vgl_simulate_tile_text_async(sim.ctx, site0, n, keep["gt"].ctypes.data, tile.byref(), keep["vt"].ctypes.data, tcap,
                                                  keep["vo"].ctypes.data, C.byref(t))
        else:
            tcap = int(lib.vgl_ctx_gvcf_text_bound(sim.ctx, S))
            G = 15
            keep.update(items=np.zeros(8 * S, np.int32), gtext=np.zeros(tcap, np.uint8), ro=np.zeros(S + 1, np.int64), bo=np.zeros(S + 1, np.int64),
                        fdp=np.zeros(N, np.int32), ldp=np.zeros(N, np.int32), fpl=np.zeros(G * N, np.int32), lpl=np.zeros(G * N, np.int32),
                        contig=np.zeros(n, np.int32), pos0=np.arange(n, dtype=np.int64) + site0, dps=np.array([1, 3, 5], np.int32))
            g = _abi.GvcfTile(keep["items"].ctypes.data, keep["gtext"].ctypes.data, tcap, keep["ro"].ctypes.data, keep["bo"].ctypes.data,
                              keep["fdp"].ctypes.data, keep["fpl"].ctypes.data, keep["ldp"].ctypes.data, keep["lpl"].ctypes.data)
            keep["g"] = g
            rc = lib.vgl_simulate_tile_gvcf_async(sim.ctx, site0, n, keep["gt"].ctypes.data, keep["contig"].ctypes.data, keep["pos0"].ctypes.data,
                                                  keep["dps"].ctypes.data, 3, tile.byref(), C.byref(g), C.byref(t))
        assert rc == _abi.VGL_OK, lib.vgl_last_error()
        subs.append((t.value, keep))
    for k in range(max(0, len(gts) - 2), len(gts)):
        wait(*subs[k])
    sim.close()
    return out


@pytest.mark.parametrize("entry", ["plain", "text", "gvcf"])
@pytest.mark.parametrize("fields", [["fmt_dp", "gl", "pl"], ["fmt_dp"]], ids=["with_gl", "without_gl"])
def test_side_channel_equals_the_model(entry, fields):
    N, S = 70, 40
    a, b = (0, 1) if entry != "gvcf" else (1, 1)
    mode = fm.TEXT if entry == "text" else fm.FLOAT
    args = sim_args(do_unobserved=2 if entry == "gvcf" else 0)
    gts = [synth.acgt_sites(S, N, seed=60 + k, missing=0.02) for k in range(2)] + [synth.acgt_sites(13, N, seed=62)]
    res = side_channel(args, N, S, gts, entry, a, b, mode, fields)
    site0 = 0
    for keep, gt in zip(res, gts):
        (want, woff), plain = model_of(args, N, site0, gt, a, b, mode)
        site0 += gt.shape[0]
        assert np.array_equal(keep["off"], woff)
        total = int(woff[-1])
        assert keep["p"].text_needed == total > 0
        assert bytes(keep["text"][:total]) == want and (keep["text"][total:] == 0x5A).all()   # only the tile's bytes were copied
        for f in fields:                                                                      # the caller's outputs are untouched
            assert np.array_equal(keep["tile"].numpy(f).view(np.uint8), plain.numpy(f).view(np.uint8)), f
        assert 0 < want.count(b"\n") <= gt.shape[0]


@pytest.mark.parametrize("layout", [_abi.VGL_LAYOUT_PLANES, _abi.VGL_LAYOUT_SAMPLE_MAJOR])
def test_simulator_interface_layouts_pairs_and_the_device_entry_point(layout):
    N, S = 65, 50
    args = sim_args(layout=layout, do_unobserved=1, depth=2)
    gt = synth.acgt_sites(S, N, seed=8, missing=0.02)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    seen = 0
    for pair, mode in (("AC", fm.FLOAT), ("CA", fm.TEXT), ("GG", fm.TEXT), ("A<", fm.FLOAT), ("<<", fm.TEXT), ("TG", fm.FLOAT)):
        a, b = fetchgl.allele_codes(pair)
        sim.fetch_gl(pair, value_mode=mode)
        tile, f = sim.simulate_fetched(5, gt, fields=["gl"] if mode == fm.FLOAT else ["fmt_dp"])
        full = sim.simulate(5, gt)                                       # no request: a plain tile
        want, woff = fm.render(full.numpy("site_status"), full.numpy("n_alleles"), full.numpy("alleles2acgt"),
                               np.ascontiguousarray(full.numpy("gl")).view(np.uint32).reshape(-1), layout, sim.G, a, b, mode)
        assert np.array_equal(f.offsets, woff) and f.text == want and f.needed == len(want), pair
        assert f.lines(np.arange(6, 6 + S)) == fm.lines(np.arange(6, 6 + S), want, woff)
        seen += want.count(b"\n")
    assert seen > 0
    # the device entry point: the caller's own device arrays through vgl_fetchgl_format_device
    dt = sim.new_tile(S, fields=["gl"], device="cuda:0")
    sim.simulate_device(5, torch.from_numpy(gt).to("cuda:0"), dt)
    sim.check()
    off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    dst = torch.zeros(fetchgl.bound(N, S), dtype=torch.uint8, device="cuda")
    fetchgl.format_into(dt["site_status"], dt["n_alleles"], dt["alleles2acgt"], dt["gl"], 3, 2, fm.FLOAT, dst, off, max_genotypes=sim.G, layout=layout)
    torch.cuda.synchronize()
    assert np.array_equal(off.cpu().numpy(), woff) and bytes(dst[:len(want)].cpu().numpy()) == want
    # switched off: a request is refused; a context without GL refuses the genotype
    sim.fetch_gl(None)
    p = _abi.FetchGlTile(None, 0, f.offsets.ctypes.data, 0)
    assert sim.lib.vgl_ctx_fetchgl_next(sim.ctx, C.byref(p)) == _abi.VGL_E_ARG
    for bad in ((5, 0, 0), (0, 5, 0), (0, -1, 0), (0, 1, 2)):
        assert sim.lib.vgl_ctx_fetchgl(sim.ctx, *bad) == _abi.VGL_E_ARG, bad
    sim.close()
    nogl = Simulator(sim_args(add_gl=0), N, device=0, max_sites_per_tile=S)
    assert nogl.lib.vgl_ctx_fetchgl(nogl.ctx, 0, 1, 0) == _abi.VGL_E_ARG and b"add_gl" in nogl.lib.vgl_last_error()
    nogl.close()


def test_serial_mode_capacity_and_the_record_loop():
    N, S = 50, 30
    gt = synth.acgt_sites(S, N, seed=4, missing=0.0)
    args = sim_args(_abi.VGL_RNG_SERIAL)
    ref = Simulator(args, N, device=0, max_sites_per_tile=S)
    full = ref.simulate(0, gt)
    G = ref.G
    ref.close()
    want, woff = fm.render(full.numpy("site_status"), full.numpy("n_alleles"), full.numpy("alleles2acgt"),
                           np.ascontiguousarray(full.numpy("gl")).view(np.uint32).reshape(-1), args.out_layout, G, 0, 0, fm.TEXT)
    res = side_channel(args, N, S, [gt], "plain", 0, 0, fm.TEXT, ["fmt_dp"])
    assert np.array_equal(res[0]["off"], woff) and bytes(res[0]["text"][: int(woff[-1])]) == want and len(want) > 0
    # a text_cap below the tile's size: VGL_E_CAPACITY, text_needed = the size, nothing written
    targs = sim_args()
    sim = Simulator(targs, N, device=0, max_sites_per_tile=S)
    sim.fetch_gl("AA")
    f = sim.fetch_next(S, text_cap=100)
    f.buf[:] = 0x5A
    tile = sim.new_tile(S, fields=["fmt_dp"])
    assert sim.lib.vgl_simulate_tile(sim.ctx, 0, S, gt.ctypes.data, tile.byref()) == _abi.VGL_E_CAPACITY
    assert f.needed > 100 and (f.buf == 0x5A).all()
    # the record loop's CSV in tiles of 7 sites equals the model over one tile
    sites = [recordloop.Site("chr1", 10 + 3 * i, gt[i], False) for i in range(S)]
    csv = recordloop.fetch_gl_csv(sim, sites, "AA", fm.TEXT, max_sites=7)
    whole = sim.simulate(0, gt)
    sim.close()
    w, wo = fm.render(whole.numpy("site_status"), whole.numpy("n_alleles"), whole.numpy("alleles2acgt"),
                      np.ascontiguousarray(whole.numpy("gl")).view(np.uint32).reshape(-1), targs.out_layout, G, 0, 0, fm.TEXT)
    assert csv == fm.lines([s.pos0 + 1 for s in sites], w, wo) and csv.count(b"\n") > 0


def test_with_a_tally_and_a_pileup_on_the_same_tile():
    N, S = 70, 40
    args = sim_args()
    gts = [synth.acgt_sites(S, N, seed=70 + k, missing=0.02) for k in range(2)]
    plain = side_channel(args, N, S, gts, "plain", 1, 0, fm.FLOAT, ["fmt_dp"])
    both = side_channel(args, N, S, gts, "plain", 1, 0, fm.FLOAT, ["fmt_dp"], also_pileup=True)
    for p, q in zip(plain, both):
        assert np.array_equal(p["off"], q["off"]) and bytes(p["text"]) == bytes(q["text"]) and q["pp"].text_needed > 0
    # with the tally on: the same text, and the table of a run without the request
    tables = []
    for req in (False, True):
        sim = Simulator(args, N, device=0, max_sites_per_tile=S)
        sim.discordance(1)
        sim.fetch_gl(1, 0, fm.FLOAT)
        if req:
            t, f = sim.simulate_fetched(0, gts[0], fields=["fmt_dp"])
            assert f.text == bytes(plain[0]["text"][:f.needed]) and f.needed > 0
        else:
            sim.simulate(0, gts[0], fields=["fmt_dp"])
        tables.append(sim.discordance_table())
        sim.close()
    assert np.array_equal(tables[0], tables[1]) and tables[0].any()


def test_a_tile_that_is_run_again_is_fetched_from_the_rerun(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (the hooks build): every tile draws deeper than the staging capacity and is run again on the
    sibling context, in sub-tiles; the text is that of the rerun's values"""
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    N, S = 100, 2500
    args = VcfglArgs(seed=42, depth=20, error_rate=0.01, add_pl=1)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    gt = synth.acgt_sites(S, N, seed=S, missing=0.03)
    sim = Simulator(args, N, max_sites_per_tile=S, hooks=True)
    assert sim.info()["read_cap"] == 8
    sim.fetch_gl("AC", value_mode=fm.TEXT)
    t, f = sim.simulate_fetched(3, gt)
    lean, f2 = sim.simulate_fetched(3, gt, fields=["fmt_dp"])
    G = sim.G
    sim.close()
    want, woff = fm.render(t.numpy("site_status"), t.numpy("n_alleles"), t.numpy("alleles2acgt"),
                           np.ascontiguousarray(t.numpy("gl")).view(np.uint32).reshape(-1), args.out_layout, G, 0, 1, fm.TEXT)
    assert int(t.numpy("fmt_dp").max()) > 8
    assert np.array_equal(f.offsets, woff) and f.text == want and len(want) > 0
    assert np.array_equal(f2.offsets, woff) and f2.text == want
    assert np.array_equal(lean.numpy("fmt_dp"), t.numpy("fmt_dp"))
