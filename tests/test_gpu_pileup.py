"""The device pileup formatter (csrc/vgl_pileup.hip: vgl_pileup_format_device, the vgl_ctx_pileup_next side channel) against the Python
model of the host writer's pileup columns (tests/pileup_model.py): synthetic tiles over every depth digit boundary, sample counts around
a wavefront and a workgroup, every site status, every read byte and the constant-score mode; the capacity contract; simulated tiles of
both RNG modes; and the record-loop side channel with two tiles in flight, alone and next to the text and gVCF entries."""
import ctypes as C

import numpy as np
import pytest
import torch

import pileup_model as pm
import synth
from vcfgl_amd import Simulator, VcfglArgs, _abi, pileup

pytestmark = pytest.mark.gpu
STATUSES = [0, 1, -3, -4]                # kept, no reads (kept), invariant (skipped), empty (no line)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synthetic(S, N, R, seed):
    """dp over 0, 1, every digit boundary up to R and random values; random read bytes (all 256 values); every site status"""
    rng = np.random.default_rng(seed)
    special = sorted({d for d in (0, 1, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, R - 1, R) if 0 <= d <= R})
    dp = rng.integers(0, min(R, 40) + 1, (S, N)).astype(np.int32)
    pick = rng.random((S, N)) < 0.3
    dp[pick] = rng.choice(special, int(pick.sum()))
    dp.reshape(-1)[: len(special)] = special[: dp.size]
    reads = rng.integers(0, 256, (R, S, N), dtype=np.uint8)
    st = np.array([STATUSES[i % 4] for i in range(S)], np.int32)
    return st, dp, reads


def check(st, dp, reads, qual_char=-1):
    N = dp.shape[1]
    text, off = pileup.format_columns(dev(st), dev(dp), dev(reads), N, qual_char=qual_char)
    want, woff = pm.render(st, dp, reads, qual=None if qual_char < 0 else qual_char)
    assert np.array_equal(off.cpu().numpy(), woff)
    got = bytes(text.cpu().numpy())
    if got != want:
        k = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        raise AssertionError(f"first difference at byte {k}: {got[max(0, k - 40):k + 40]!r} vs {want[max(0, k - 40):k + 40]!r}")
    return got


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 2500])
def test_synthetic_tiles_equal_the_model(N):
    R = 1020 if N <= 65 else 120
    S = {1: 300, 63: 40, 64: 40, 65: 40, 1000: 8, 2500: 4}[N]
    st, dp, reads = synthetic(S, N, R, seed=N)
    got = check(st, dp, reads)
    assert got.count(b"\n") == int((st != -4).sum())


@pytest.mark.parametrize("qc", [33, ord("5"), 32, 0, 255])
def test_constant_score_mode(qc):
    st, dp, reads = synthetic(12, 65, 140, seed=qc)
    check(st, dp, reads, qual_char=qc)


def test_every_read_byte_and_digit_boundary():
    # 256 samples with one read each (read byte = the sample index), then one sample that reads all 256 values at depth 256
    R = 1020
    dp = np.ones((3, 256), np.int32)
    reads = np.zeros((R, 3, 256), np.uint8)
    reads[0, 0, :] = np.arange(256)
    dp[1, :] = 0
    dp[1, 7] = 256
    reads[:256, 1, 7] = np.arange(256)
    dp[2, :10] = [0, 1, 9, 10, 99, 100, 999, 1000, 1019, 1020]
    reads[:, 2, :] = np.random.default_rng(3).integers(0, 256, (R, 256), dtype=np.uint8)
    check(np.zeros(3, np.int32), dp, reads)


def test_unaligned_destinations_and_capacity_contract():
    st, dp, reads = synthetic(30, 77, 50, seed=9)
    N = dp.shape[1]
    text, off = pileup.format_columns(dev(st), dev(dp), dev(reads), N)
    total = int(off[-1])
    assert total == text.numel() > 0
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for shift in (1, 2, 3, 5):                                   # a destination that starts off a dword boundary
        buf.fill_(0xA5)
        dst = buf[shift:]
        o = pileup.format_into(dev(st), dev(dp), dev(reads), N, dst, dst_cap=total)
        torch.cuda.synchronize()
        assert torch.equal(o, off) and torch.equal(dst[:total], text)
        assert bool((buf[:shift] == 0xA5).all()) and bool((dst[total:] == 0xA5).all())
    buf.fill_(0xA5)
    o = pileup.format_into(dev(st), dev(dp), dev(reads), N, buf, dst_cap=total - 1)
    torch.cuda.synchronize()
    assert int(o[-1]) == total and bool((buf == 0xA5).all())     # too small: the size it needs, nothing written
    # a depth beyond the dump's capacity (or below 0): offsets[n] = -1, nothing written, and no row at or beyond the capacity is read
    for bad in (51, -1):
        dp2 = dp.copy()
        dp2[17, 40] = bad
        o = pileup.format_into(dev(st), dev(dp2), dev(reads), N, buf)
        torch.cuda.synchronize()
        assert int(o[-1]) == -1 and bool((buf == 0xA5).all())
        with pytest.raises(ValueError):
            pileup.format_columns(dev(st), dev(dp2), dev(reads), N)
    lib = _abi.load_library()
    assert lib.vgl_pileup_format_device(0, N, 30, dev(st).data_ptr(), dev(dp).data_ptr(), dev(reads).data_ptr(), 50, -1, buf.data_ptr(),
                                        buf.numel(), o.data_ptr(), None, 0, None) == _abi.VGL_E_ARG          # no workspace
    assert lib.vgl_pileup_format_device(0, N, 30, None, None, None, 50, 300, None, 0, None, None, 0, None) == _abi.VGL_E_ARG
    # no sites: offsets[0] = 0
    o0 = pileup.format_into(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                            torch.zeros((5, 0, N), dtype=torch.uint8, device="cuda"), N, buf)
    assert int(o0[-1]) == 0


def sim_args(mode, **kw):
    base = dict(seed=11, depth=6, error_rate=0.02, add_fmt_dp=1, add_pl=1, out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR)
    base.update(kw)
    a = VcfglArgs(**base)
    a.rng_mode = mode
    a.beta_sampler = _abi.VGL_BETA_STD if mode == _abi.VGL_RNG_SERIAL else _abi.VGL_BETA_RAND48
    return a


@pytest.mark.parametrize("mode", [_abi.VGL_RNG_TILE, _abi.VGL_RNG_SERIAL])
@pytest.mark.parametrize("kw", [{}, dict(error_qs=2, beta_variance=1e-4, rm_empty_sites=1, depth=0.02), dict(depth=25, do_unobserved=4)])
def test_simulated_device_tiles_equal_the_model(mode, kw):
    N, S = 130, 48
    args = sim_args(mode, **kw)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    cap = sim.info()["read_cap"]
    tile = sim.new_tile(S, fields=["fmt_dp"], device="cuda:0", read_capacity=cap)
    gt = synth.acgt_sites(S, N, seed=5, missing=0.02)
    sim.simulate_device(0, dev(gt), tile)
    sim.check()
    st, dp, reads = tile.numpy("site_status"), tile.numpy("fmt_dp"), tile.numpy("reads")
    assert dp.max() > 0 and dp.max() <= cap
    check(st, dp, reads)
    if kw.get("rm_empty_sites"):
        assert (st == -4).any()
    sim.close()


def reference_pileup(args, N, site0, gt, qual):
    """the host path: the tile simulated with a host read dump (and deviates), rendered by the model"""
    sim = Simulator(args, N, device=0, max_sites_per_tile=gt.shape[0])
    cap = sim.info()["read_cap"]
    tile = sim.simulate(site0, gt, fields=["fmt_dp"], read_capacity=cap, deviates=args.error_qs == 2)
    sim.close()
    q = None
    if qual == "errp":
        ep = tile.numpy("read_errp")
        with np.errstate(invalid="ignore"):                         # (rows past a sample's depth hold NaN)
            q = np.vectorize(lambda e: pm.adjusted_score(float(e), args.adjust_by) if 0 <= e <= 1 else 0)(ep)
    elif qual is not None:
        q = qual
    return pm.render(tile.numpy("site_status"), tile.numpy("fmt_dp"), tile.numpy("reads"), qual=q)


def side_channel(args, N, S, gts, entry):
    """vgl_ctx_pileup_next + one of the three async entries for consecutive tiles, two in flight: tile k + 2 is submitted after tile k's wait"""
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    lib = sim.lib
    cap = int(lib.vgl_ctx_pileup_bound(sim.ctx, S))
    assert cap == pileup.bound(N, S, sim.info()["read_cap"])
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
        p = _abi.PileupTile(keep["text"].ctypes.data, cap, keep["off"].ctypes.data, -7)
        keep["p"] = p
        tile = sim.new_tile(n, fields=["fmt_dp"])
        keep["tile"] = tile
        sim._check(lib.vgl_ctx_pileup_next(sim.ctx, C.byref(p)))
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
    # a tile without a request has no pileup: the request is taken by one tile only
    tile = sim.new_tile(gts[0].shape[0], fields=["fmt_dp"])
    sim._check(lib.vgl_simulate_tile(sim.ctx, 10 ** 5 if args.rng_mode == _abi.VGL_RNG_TILE else sum(g.shape[0] for g in gts),
                                     gts[0].shape[0], np.ascontiguousarray(gts[0]).ctypes.data, tile.byref()))
    sim.close()
    return out


@pytest.mark.parametrize("entry", ["plain", "text", "gvcf"])
@pytest.mark.parametrize("kw,qual", [({}, None), (dict(adjust_qs=4, error_rate=0.013), "const"),
                                     (dict(adjust_qs=4, error_qs=2, beta_variance=1e-3), "errp"),
                                     (dict(error_qs=1, beta_variance=1e-4, rm_empty_sites=1, depth=0.8), None)])
def test_record_loop_side_channel_equals_the_model(entry, kw, qual):
    N, S = 70, 40
    args = sim_args(_abi.VGL_RNG_TILE, **kw)
    gts = [synth.acgt_sites(S, N, seed=60 + k, missing=0.02) for k in range(2)] + [synth.acgt_sites(13, N, seed=62)]
    res = side_channel(args, N, S, gts, entry)
    q = None
    if qual == "const":
        q = pm.adjusted_score(args.error_rate, args.adjust_by) + 33
    site0 = 0
    for keep, gt in zip(res, gts):
        want, woff = reference_pileup(args, N, site0, gt, "errp" if qual == "errp" else q)
        site0 += gt.shape[0]
        assert np.array_equal(keep["off"], woff)
        total = int(woff[-1])
        assert keep["p"].text_needed == total > 0
        assert bytes(keep["text"][:total]) == want and (keep["text"][total:] == 0x5A).all()   # only the tile's bytes were copied
        if entry == "text":
            assert int(keep["vo"][-1]) > 0
        if entry == "gvcf":
            assert keep["g"].n_items > 0


def test_side_channel_capacity_and_serial_mode():
    N, S = 50, 30
    gt = synth.acgt_sites(S, N, seed=4, missing=0.0)
    # serial mode: one tile through the side channel equals the host path
    args = sim_args(_abi.VGL_RNG_SERIAL)
    res = side_channel(args, N, S, [gt], "plain")
    want, woff = reference_pileup(args, N, 0, gt, None)
    assert np.array_equal(res[0]["off"], woff) and bytes(res[0]["text"][: int(woff[-1])]) == want
    # a text_cap below the tile's size: VGL_E_CAPACITY, text_needed = the size, nothing written
    args = sim_args(_abi.VGL_RNG_TILE)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    lib = sim.lib
    buf, off = np.full(4096, 0x5A, np.uint8), np.zeros(S + 1, np.int64)
    p = _abi.PileupTile(buf.ctypes.data, 1000, off.ctypes.data, 0)
    assert lib.vgl_ctx_pileup_next(sim.ctx, C.byref(p)) == _abi.VGL_OK
    tile = sim.new_tile(S, fields=["fmt_dp"])
    assert lib.vgl_simulate_tile(sim.ctx, 0, S, gt.ctypes.data, tile.byref()) == _abi.VGL_E_CAPACITY
    assert p.text_needed > 1000 and (buf == 0x5A).all()
    bad = _abi.PileupTile(None, 10, None, 0)
    assert lib.vgl_ctx_pileup_next(sim.ctx, C.byref(bad)) == _abi.VGL_E_ARG
    sim.close()
