"""Record streams on the device (csrc/vgl_stream.hip: vgl_stream_assemble_device, vgl_stream_host_*; vgl_ctx_text_device) against the
numpy model (tests/stream_model.py), byte for byte: every alignment of the three buffers, both ends of the work decomposition (thousands
of tiny records, a few of 300 KB), the capacity contract, offsets beyond 2^31, the host handle (members equal to the BGZF model's), and
tiles delivered to a device destination."""
import ctypes as C

import numpy as np
import pytest
import torch

import bcf_reader
import bgzf_model
import stream_model as sm
import synth
import test_gpu_bcf as tb
import test_gpu_vcftext as tt
from vcfgl_amd import Simulator, VcfglArgs, _abi, stream

pytestmark = pytest.mark.gpu
M = bgzf_model.MEMBER
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
GUARD = 64


def offsets_of(lengths, base=0):
    return np.concatenate([[base], base + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def random_tile(rng, head_len, body_len, text=False):
    """heads / bodies of the given per-site lengths: random bytes, or record-like text (what compresses)"""
    def fill(n):
        if not text:
            return rng.integers(0, 256, n, dtype=np.uint8)
        words = [b"0/0", b"0/1", b"1/1", b"-0.30103", b"\t", b"\n", b"PASS", b"chr1", b":", b"17"]
        s = b"".join(words[i] for i in rng.integers(0, len(words), n // 2 + 8))
        return np.frombuffer(s[:n], dtype=np.uint8).copy()
    return fill(int(np.sum(head_len))), offsets_of(head_len), fill(int(np.sum(body_len))), offsets_of(body_len)


def run(heads, ho, bodies, bo, sh=0, sb=0, sd=0, cap=None, base_h=0, base_b=0):
    """the device stream of a tile whose buffers start sh / sb / sd bytes into their tensors; dst between guards of 0xA5.
    Returns (total, stream bytes, whole dst tensor on the host)"""
    want, _ = sm.assemble(heads, ho, bodies, bo)
    n = len(want)
    dh = torch.from_numpy(np.concatenate([np.zeros(sh, np.uint8), heads, np.zeros(8, np.uint8)])).cuda()[sh:]
    db = torch.from_numpy(np.concatenate([np.zeros(sb, np.uint8), bodies, np.zeros(8, np.uint8)])).cuda()[sb:]
    whole = torch.full((GUARD + sd + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = whole[GUARD + sd:GUARD + sd + max(n, 1)]
    assert dh.data_ptr() % 4 == sh and db.data_ptr() % 4 == sb and dst.data_ptr() % 4 == sd
    total = stream.assemble_into(dh, torch.from_numpy(ho + base_h).cuda(), db, torch.from_numpy(bo + base_b).cuda(), dst,
                                 dst_cap=n if cap is None else cap)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    return int(total.item()), want, w, GUARD + sd


def check(heads, ho, bodies, bo, **kw):
    total, want, w, at = run(heads, ho, bodies, bo, **kw)
    assert total == len(want)
    assert (w[:at] == 0xA5).all() and (w[at + total:] == 0xA5).all(), "guard bytes were written"
    assert bytes(w[at:at + total]) == bytes(want)
    return want


LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65]


@pytest.fixture(scope="module")
def sweep_tile():
    rng = np.random.default_rng(5)
    hl = rng.choice(LENGTHS, 64)
    bl = rng.choice(LENGTHS, 64)
    bl[[9, 30, 51]] = [1000, 4099, 70001]
    hl[[3, 4]] = 0
    bl[[3, 4]] = 0                                                    # two sites that contribute nothing
    assert set(LENGTHS) <= set(hl) | set(bl)
    return random_tile(rng, hl, bl)


@pytest.mark.parametrize("sd", [0, 1, 2, 3])
def test_alignment_sweep(sweep_tile, sd):
    """64 sites whose head and body lengths cover 0 .. 65 around the 4- and 16-byte steps plus bodies of 1000, 4099 and 70001 bytes;
    heads, bodies and dst each 0 - 3 bytes into their tensors (all 64 combinations); offsets that start at another value than 0"""
    for sh in range(4):
        for sb in range(4):
            check(*sweep_tile, sh=sh, sb=sb, sd=sd, base_h=17 * sh, base_b=1000003 * sb)


def test_thousands_of_tiny_records():
    rng = np.random.default_rng(6)
    check(*random_tile(rng, rng.integers(12, 31, 4096), rng.integers(5, 10, 4096)), sh=1, sb=2, sd=3)


def test_three_records_of_300_kb():
    rng = np.random.default_rng(7)
    check(*random_tile(rng, [40, 37, 45], [300001, 299999, 300123]), sh=3, sb=1, sd=2)


def test_no_site_and_only_empty_sites():
    e = np.zeros(0, np.uint8)
    assert run(e, offsets_of([]), e, offsets_of([]))[0] == 0
    # every site empty, at every alignment of dst (off a 16-byte boundary the first piece is not empty by its address alone); the
    # offsets tensors hold exactly n_sites + 1 entries
    for sd in range(4):
        for n in (1, 9, 300):
            total, want, w, at = run(e, offsets_of([0] * n), e, offsets_of([0] * n), sd=sd, base_h=5, base_b=7)
            assert total == 0 and len(want) == 0 and (w == 0xA5).all(), (sd, n)


def test_capacity_one_byte_short_writes_nothing(sweep_tile):
    want, _ = sm.assemble(*sweep_tile)
    total, _, w, at = run(*sweep_tile, sd=1, cap=len(want) - 1)
    assert total == len(want)                                         # the size it needs is reported
    assert (w == 0xA5).all()                                          # nothing written
    check(*sweep_tile, sd=1, cap=len(want))


def test_offsets_beyond_2_to_the_31():
    """a bodies tensor just over 2^31 bytes whose second site's body starts beyond 2^31; compared on the device"""
    big = (1 << 31) + 4099
    g = torch.Generator(device="cuda").manual_seed(8)
    bodies = torch.empty(big + 1000 + 1, dtype=torch.uint8, device="cuda")
    for a in range(0, bodies.numel(), 1 << 28):                       # (filled in pieces: random bytes)
        piece = bodies[a:a + (1 << 28)]
        piece.copy_(torch.randint(0, 256, (piece.numel(),), dtype=torch.uint8, device="cuda", generator=g))
    heads = torch.randint(0, 256, (77,), dtype=torch.uint8, device="cuda", generator=g)
    ho = torch.tensor([0, 33, 77], dtype=torch.int64, device="cuda")
    bo = torch.tensor([1, 1 + big, 1 + big + 1000], dtype=torch.int64, device="cuda")      # bodies[1:]: an odd source
    n = 77 + big + 1000
    whole = torch.full((GUARD + 3 + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = whole[GUARD + 3:GUARD + 3 + n]
    total = stream.assemble_into(heads, ho, bodies[1:], bo, dst)
    torch.cuda.synchronize()
    assert int(total.item()) == n > 1 << 31
    assert bool((whole[:GUARD + 3] == 0xA5).all()) and bool((whole[GUARD + 3 + n:] == 0xA5).all())
    j1 = 33 + big                                                     # where record 1 starts
    assert torch.equal(dst[:33], heads[:33]) and torch.equal(dst[33:33 + 5000], bodies[1:5001])
    assert torch.equal(dst[j1 - 5000:j1], bodies[1 + big - 5000:1 + big])
    assert torch.equal(dst[j1:j1 + 44], heads[33:]) and torch.equal(dst[j1 + 44:], bodies[1 + big:1 + big + 1000])
    at31 = (1 << 31) - 33                                             # around the 2^31st byte of the destination
    assert torch.equal(dst[(1 << 31) - 70000:(1 << 31) + 4000], bodies[1 + at31 - 70000:1 + at31 + 4000])
    assert torch.equal(dst[33:j1], bodies[1:1 + big])                 # the whole of body 0


def to_raw(ptr, t):
    """copy the device tensor t to the raw device address ptr (a one-site stream: no head, t as the body)"""
    z = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, t.numel()], dtype=torch.int64, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib = _abi.load_library()
    assert lib.vgl_stream_assemble_device(0, 1, t.data_ptr(), z.data_ptr(), t.data_ptr(), off.data_ptr(), ptr, t.numel(), total.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream) == _abi.VGL_OK
    torch.cuda.synchronize()
    assert int(total.item()) == t.numel()


def members_ok(members, want):
    """header, CRC and size of every member; what they decompress to"""
    blocks = bcf_reader.bgzf_blocks(members + EOF)
    assert b"".join(blocks) == bytes(want)
    assert [len(b) for b in blocks[:-1]] == [M] * (len(want) // M) + ([len(want) % M] if len(want) % M else [])


def test_host_handle():
    """two tickets in flight waited in order, members equal to the BGZF model's for streams of two to three members, a buffer used
    again after its wait, a submit on a buffer in flight, bad arguments, an empty tile"""
    rng = np.random.default_rng(9)
    S = 500
    tiles = []
    for k, raw in enumerate((2 * M + 1, 3 * M + 100 - 7, 2 * M + 999)):
        hl = rng.integers(20, 40, S)
        bl = rng.integers(100, 200, S)
        bl[-1] += raw - int(hl.sum() + bl.sum())
        assert bl[-1] > 0
        tiles.append(random_tile(rng, hl, bl, text=True))
    max_head, max_body = 40 * S, 3 * M + 100
    with stream.HostStream(0, 2, S, max_head, max_body) as hs:
        lib = hs.lib
        assert hs.body(0) and hs.body(1) and hs.body(0) != hs.body(1)
        assert not lib.vgl_stream_host_body(hs.h, 2) and not lib.vgl_stream_host_body(hs.h, -1)
        for k in (0, 1):
            to_raw(hs.body(k), torch.from_numpy(tiles[k][2]).cuda())
        t0 = hs.submit(0, tiles[0][0], tiles[0][1], tiles[0][3])
        t1 = hs.submit(1, tiles[1][0], tiles[1][1], tiles[1][3])
        assert t0 != t1
        rc, _ = hs.submit_rc(0, tiles[0][0], tiles[0][1], tiles[0][3])          # buffer 0 is in flight
        assert rc == _abi.VGL_E_ARG and b"in flight" in lib.vgl_last_error()
        p, n = C.c_void_p(), C.c_int64()
        assert lib.vgl_stream_host_wait(hs.h, t1, C.byref(p), C.byref(n), None) == _abi.VGL_E_ARG and b"submit order" in lib.vgl_last_error()
        for k, t in ((0, t0), (1, t1)):
            members, raw_n = hs.wait(t)
            want, _ = sm.assemble(*tiles[k])
            assert raw_n == len(want)
            members_ok(members, want)
            assert members == bgzf_model.compress(bytes(want)), k
            assert lib.vgl_stream_host_wait(hs.h, t, C.byref(p), C.byref(n), None) == _abi.VGL_E_ARG        # already waited
        # buffer 0 again, with other bytes
        to_raw(hs.body(0), torch.from_numpy(tiles[2][2]).cuda())
        members, raw_n = hs.wait(hs.submit(0, tiles[2][0], tiles[2][1], tiles[2][3]))
        want, _ = sm.assemble(*tiles[2])
        members_ok(members, want)
        assert members == bgzf_model.compress(bytes(want))
        # offsets that do not start at 0: submit indexes `heads` and the body buffer absolutely -- head i is heads[ho[i] .. ho[i + 1]),
        # body i is bytes [bo[i], bo[i + 1]) of buffer k
        heads2, ho2, bodies2, bo2 = tiles[1]
        pre = np.full(5, 0xEE, np.uint8)
        to_raw(hs.body(1) + 7, torch.from_numpy(bodies2[:M]).cuda())
        bo2 = np.minimum(bo2, M)                                      # (the first 0xff00 bytes of the bodies: it fits behind the shift)
        members, raw_n = hs.wait(hs.submit(1, np.concatenate([pre, heads2]), ho2 + 5, bo2 + 7))
        want, _ = sm.assemble(heads2, ho2, bodies2[:M], bo2)
        assert raw_n == len(want)
        members_ok(members, want)
        # an empty tile, and a tile of empty sites
        e = np.zeros(1, np.uint8)
        assert hs.wait(hs.submit(1, e, offsets_of([]), offsets_of([]))) == (b"", 0)
        assert hs.wait(hs.submit(1, e, offsets_of([0, 0, 0]), offsets_of([0, 0, 0]))) == (b"", 0)
        # bad arguments: refused with a message that names the argument, and nothing is left in flight
        heads, ho, _, bo = tiles[0]
        down = ho.copy()
        down[5] = down[4] - 1
        for args, word in (((2, heads, ho, bo), b"k is out of range"), ((-1, heads, ho, bo), b"k is out of range"),
                           ((0, heads, down, bo), b"head_offsets"), ((0, heads, ho, down), b"body_offsets"),
                           ((0, heads, offsets_of([max_head + 1]), offsets_of([5])), b"max_head_bytes"),
                           ((0, heads, offsets_of([5]), offsets_of([max_body + 1])), b"max_body_bytes"),
                           ((0, heads, offsets_of([1] * (S + 1)), offsets_of([1] * (S + 1))), b"n_sites")):
            rc, _ = hs.submit_rc(*args)
            assert rc == _abi.VGL_E_ARG and word in lib.vgl_last_error(), (word, lib.vgl_last_error())
        assert hs.wait(hs.submit(0, e, offsets_of([]), offsets_of([]))) == (b"", 0)
    h = C.c_void_p()
    assert lib.vgl_stream_host_create(0, 0, S, 10, 10, C.byref(h)) == _abi.VGL_E_ARG and b"n_buffers" in lib.vgl_last_error()
    assert lib.vgl_stream_host_create(1 << 20, 2, S, 10, 10, C.byref(h)) == _abi.VGL_E_NODEVICE


def ctx_text_device(sim, site0, gts, text_cap=None):
    """tt.ctx_text with device destinations (vgl_ctx_text_device): [(rc, device buffer, host offsets, tile)]"""
    lib = sim.lib
    cap = int(lib.vgl_ctx_text_bound(sim.ctx, sim.max_sites_per_tile))
    sim._check(lib.vgl_ctx_text_device(sim.ctx, 1))
    subs = []
    for k, gt in enumerate(gts):
        tile = sim.new_tile(gt.shape[0], fields=["fmt_dp"])
        buf = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        off = np.zeros(gt.shape[0] + 1, dtype=np.int64)
        t = C.c_int32()
        gt = np.ascontiguousarray(gt)
        sim._check(lib.vgl_simulate_tile_text_async(sim.ctx, site0 + sum(g.shape[0] for g in gts[:k]), gt.shape[0], gt.ctypes.data, tile.byref(),
                                                     buf.data_ptr(), cap if text_cap is None else text_cap, off.ctypes.data, C.byref(t)))
        subs.append((t.value, buf, off, tile, gt))
    out = [(lib.vgl_tile_wait(sim.ctx, t), buf.cpu().numpy(), off, tile) for t, buf, off, tile, gt in subs]
    assert lib.vgl_ctx_text_device(sim.ctx, 0) == _abi.VGL_OK
    return out


@pytest.mark.parametrize("bcf", [False, True])
def test_tiles_delivered_to_a_device_buffer(bcf):
    """the tiles of test_gpu_vcftext's two-in-flight case: a device destination receives the bytes and offsets the host destination
    receives, as text and (vgl_ctx_bcf_keys) as typed vectors; the capacity contract holds; switching back restores the host path"""
    N, S = 300, 64
    sim, _, _ = tt.simulate_tile(VcfglArgs(seed=21, depth=5, error_rate=0.01, do_unobserved=2, **tt.ALL), N, S)
    if bcf:
        tb.set_keys(sim)
    gts = [synth.acgt_sites(S, N, seed=40 + k, missing=0.03) for k in range(2)]
    host = tt.ctx_text(sim, 100, gts)
    dev = ctx_text_device(sim, 100, gts)
    for (rc0, b0, o0, t0), (rc1, b1, o1, t1) in zip(host, dev):
        assert rc0 == rc1 == _abi.VGL_OK, sim.lib.vgl_last_error()
        total = int(o0[-1])
        assert total > 0 and np.array_equal(o0, o1)
        assert bytes(b1[:total]) == bytes(b0[:total]) and (b1[total:] == 0x5A).all()
        assert (b1[0] == 0x11 and b1[1] == tb.IDS["DP"]) if bcf else bytes(b1[:3]) == b"\tDP"
        for f in ("site_status", "n_alleles", "fmt_dp"):
            assert np.array_equal(t0.numpy(f), t1.numpy(f)), f
    rc, buf, off, _ = ctx_text_device(sim, 100, gts[:1], text_cap=1000)[0]
    assert rc == _abi.VGL_E_CAPACITY and int(off[-1]) > 1000 and (buf == 0x5A).all()
    rc, buf, off, _ = tt.ctx_text(sim, 100, gts[:1])[0]                # the host destination again
    assert rc == _abi.VGL_OK and bytes(buf[:int(off[-1])]) == bytes(host[0][1][:int(off[-1])])
    assert sim.lib.vgl_ctx_text_device(None, 1) == _abi.VGL_E_ARG
    sim.close()


def test_deep_rerun_is_delivered_to_the_device_buffer(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (hooks build), as test_gpu_vcftext's rerun test: every tile is run and formatted again by
    vgl_tile_wait, into the device destination"""
    N, S = 100, 40
    gts = [synth.acgt_sites(S, N, seed=70 + k, missing=0.03) for k in range(2)]

    def mk(hooks):
        args = VcfglArgs(seed=42, depth=20, error_rate=0.01, add_pl=1, add_fmt_ad=1)
        args.rng_mode, args.beta_sampler, args.out_layout = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48, _abi.VGL_LAYOUT_SAMPLE_MAJOR
        return Simulator(args, N, max_sites_per_tile=S, hooks=hooks)

    sim = mk(False)
    plain = tt.ctx_text(sim, 3, gts)
    sim.close()
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    sim = mk(True)
    assert sim.info()["read_cap"] == 8
    deep = ctx_text_device(sim, 3, gts)
    sim.close()
    for (rc0, b0, o0, t0), (rc1, b1, o1, t1) in zip(plain, deep):
        assert rc0 == rc1 == _abi.VGL_OK
        assert np.array_equal(o0, o1) and bytes(b0[:o0[-1]]) == bytes(b1[:o1[-1]]) and (b1[o1[-1]:] == 0x5A).all()
        assert np.array_equal(t0.numpy("fmt_dp"), t1.numpy("fmt_dp")) and int(t1.numpy("fmt_dp").max()) > 8
