"""The device BCF encoder (csrc/vgl_bcf.hip: vgl_bcf_encode_device, vgl_ctx_bcf_keys) against the numpy model of the host writer's FORMAT
bytes (tests/bcf_model.py), byte for byte and offset for offset: the integer-type thresholds at the first, a middle and the last sample
of a site, 1 to 2500 samples, 1 to 5 alleles mixed within a tile, skipped sites, float bit patterns, every count kind, up to 7 fields,
the capacity contract, and whole simulated tiles through the record-loop entries (plain records, gVCF, a deep re-run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bcf_model as bm
import synth
import test_gpu_gvcf as tg
import test_gpu_vcftext as tt
from vcfgl_amd import Simulator, VcfglArgs, _abi, bcfenc, gvcf

pytestmark = pytest.mark.gpu
M, E = bm.INT32_MISSING, bm.INT32_VEND
# dictionary ids of DP, GL, PL, GP, AD, ADF, ADR: every width of the typed key
IDS = dict(DP=0, GL=127, PL=128, GP=32767, AD=32768, ADF=5, ADR=70000)
KEY_IDS = [IDS[k] for k in bcfenc.KEY_ORDER]


def device_encode(fields, st, na, N):
    dfields = [(k, torch.from_numpy(a).cuda(), kind) for k, a, kind in fields]
    data, off = bcfenc.encode_records(dfields, torch.from_numpy(st).cuda(), torch.from_numpy(na).cuda(), N)
    return bytes(data.cpu().numpy()), off.cpu().numpy()


def check(fields, st, na, N):
    want, woff = bm.encode(fields, st, na, N)
    got, off = device_encode(fields, st, na, N)
    assert np.array_equal(off, woff)
    if got != want:
        i = next(k for k in range(len(want)) if got[k] != want[k])
        site = int(np.searchsorted(woff, i, side="right")) - 1
        raise AssertionError(f"first difference at byte {i} (site {site}, {i - woff[site]} into it): {got[i]:#x} != {want[i]:#x}")
    return want, woff


def corpus_tile(N, seed):
    """45 kept sites (each threshold vector at the first, a middle and the last sample) with skipped sites between them, nA 1 .. 5 mixed,
    seven fields: the vector's values in PL and AD, its first threshold value in DP; NaN payloads and the missing pattern in GL / GP"""
    rng = np.random.default_rng(seed)
    vecs = bm.threshold_vectors()
    S = 3 * len(vecs) + 6
    na = (1 + (np.arange(S) * 3 + seed) % 5).astype(np.int32)
    st = np.zeros(S, dtype=np.int32)
    st[::9] = -3                                                     # skipped sites, the first one among them
    st[-1] = 1                                                       # (a no-reads site is kept)
    dp = rng.integers(0, 100, (S, N)).astype(np.int32)
    pl = rng.integers(0, 100, (S, N * 15)).astype(np.int32)
    ad = rng.integers(0, 100, (S, N * 5)).astype(np.int32)
    adf = rng.integers(0, 300, (S, N * 5)).astype(np.int32)
    adr = rng.integers(0, 3, (S, N * 5)).astype(np.int32)
    gl = rng.standard_normal((S, N * 15)).astype(np.float32)
    gp = rng.random((S, N * 15)).astype(np.float32)
    gl.view(np.uint32)[:, ::7] = bm.FLOAT_MISSING_BITS
    gl.view(np.uint32)[:, 3::11] = 0x7FC12345                        # NaN payloads, -0
    gp.view(np.uint32)[:, 1::5] = 0xFFC00001
    gp.view(np.uint32)[:, 2::13] = 0x80000000
    k = 0
    for i in range(S):
        if st[i] < 0:
            continue
        name, v = vecs[k % len(vecs)]
        s = [0, N // 2, N - 1][(k // len(vecs)) % 3]
        k += 1
        nA = int(na[i]); nG = nA * (nA + 1) // 2
        ordinary = [x for x in v if x not in (M, E)]
        dp[i, s] = ordinary[-2] if len(ordinary) >= 2 else v[0]       # [0, t, 5]: the threshold; a special vector: its first value
        head = ([v[1], v[0]] + list(v[2:])) if len(v) > 1 else list(v)   # the threshold first: it stays when nG = 1
        for j in range(min(nG, len(head))):
            pl[i, s * nG + j] = head[j]
        for j in range(min(nA, len(head))):
            ad[i, s * nA + j] = head[j]
        if name in ("all missing", "only vector end"):                # the whole vector without an ordinary value
            pl[i, :] = v[0]
            adr[i, :] = v[0]
    fields = [(IDS["DP"], dp, bm.ONE), (IDS["GL"], gl, bm.PER_G), (IDS["PL"], pl, bm.PER_G), (IDS["GP"], gp, bm.PER_G),
              (IDS["AD"], ad, bm.PER_A), (IDS["ADF"], adf, bm.PER_A), (IDS["ADR"], adr, bm.PER_A)]
    return fields, st, na


@pytest.mark.parametrize("N", [1, 3, 7, 60, 65, 1000, 2500])
def test_threshold_corpus_equals_the_model(N):
    fields, st, na = corpus_tile(N, seed=N)
    want, off = check(fields, st, na, N)
    assert off[0] == off[1] == 0 and off[-1] == len(want) > 0        # the skipped first site has no bytes
    types = {bm.int_type(a[i, :bm.values_of(kind, int(na[i]), a.shape[1], N) * N]) for _, a, kind in fields if a.dtype == np.int32
             for i in range(len(st)) if st[i] >= 0}
    assert types == {1, 2, 3}
    assert (na == 5).any() and (na == 1).any()


@pytest.mark.parametrize("nf", [0, 1, 2, 3])
def test_each_count_kind_alone_and_no_field(nf):
    """one field of each count kind (and none at all: every kept site is empty), odd strides so that slabs are not 16-byte aligned"""
    N, S = 13, 70
    rng = np.random.default_rng(nf)
    na = rng.integers(1, 6, S).astype(np.int32)
    st = np.where(rng.random(S) < 0.2, -4, 0).astype(np.int32)
    kinds = {1: (bm.ONE, N + 1), 2: (bm.PER_G, N * 15 + 3), 3: (bm.PER_A, N * 5 + 1)}
    fields = []
    if nf:
        kind, stride = kinds[nf]
        fields = [(nf, rng.integers(-200, 200, (S, stride)).astype(np.int32), kind)]
    want, off = check(fields, st, na, N)
    assert (len(want) == 0) == (nf == 0)


def test_a_slab_narrower_than_the_site_gives_fewer_values():
    """site_stride / N bounds n(i): a PER_G field with room for 3 values per sample at 5 alleles, and one with room for none (n = 0: the
    type byte alone)"""
    N, S = 4, 9
    rng = np.random.default_rng(2)
    na = np.full(S, 5, dtype=np.int32)
    st = np.zeros(S, dtype=np.int32)
    fields = [(1, rng.integers(0, 50, (S, 3 * N)).astype(np.int32), bm.PER_G), (2, rng.integers(0, 50, (S, N - 1)).astype(np.int32), bm.PER_A),
              (3, rng.random((S, N - 1)).astype(np.float32), bm.ONE)]
    want, off = check(fields, st, na, N)
    assert want[:off[1]][-6:] == bytes([0x11, 2, 0x01, 0x11, 3, 0x05]) and off[1] == 2 + 1 + 3 * N + 6


def test_capacity_one_byte_short_writes_nothing():
    N = 65
    fields, st, na = corpus_tile(N, seed=4)
    want, woff = bm.encode(fields, st, na, N)
    total = len(want)
    dfields = [(k, torch.from_numpy(a).cuda(), kind) for k, a, kind in fields]
    dst_st, dna = torch.from_numpy(st).cuda(), torch.from_numpy(na).cuda()
    assert bcfenc.bound(dfields, len(st), N) >= total
    dst = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    o2 = bcfenc.encode_into(dfields, dst_st, dna, N, dst, dst_cap=total - 1)
    torch.cuda.synchronize()
    assert int(o2[-1]) == total                                    # the size it needs is reported
    assert bool((dst == 0xA5).all())                               # nothing written
    o3 = bcfenc.encode_into(dfields, dst_st, dna, N, dst, dst_cap=total)
    torch.cuda.synchronize()
    assert np.array_equal(o3.cpu().numpy(), woff) and bytes(dst[:total].cpu().numpy()) == want and bool((dst[total:] == 0xA5).all())
    # an odd destination: every site's head and tail bytes move
    o4 = bcfenc.encode_into(dfields, dst_st, dna, N, dst[1:], dst_cap=total)
    torch.cuda.synchronize()
    assert bytes(dst[1:total + 1].cpu().numpy()) == want and int(dst[0]) == want[0] and bool((dst[total + 1:] == 0xA5).all())
    lib = _abi.load_library()
    bad = (_abi.BcfField * 1)(_abi.BcfField(1, 0, 7, dfields[0][1].data_ptr(), 1))
    assert lib.vgl_bcf_encode_device(0, bad, 1, N, len(st), dst_st.data_ptr(), dna.data_ptr(), dst.data_ptr(), dst.numel(), o3.data_ptr(), None, 0,
                                     None) == _abi.VGL_E_ARG
    assert lib.vgl_bcf_bound(-1, 1, bad, 1, 5) == -1 and lib.vgl_bcf_workspace_bytes(1, -1) == -1


def set_keys(sim, ids=KEY_IDS):
    arr = (C.c_int32 * 7)(*ids) if ids is not None else None
    sim._check(sim.lib.vgl_ctx_bcf_keys(sim.ctx, arr, 7))


def model_of_tile(args, tile, N, st=None):
    fields = [(IDS[key], tile.numpy(name).reshape(tile.n_sites, -1), kind) for key, name, _, kind, flag in bcfenc.FORMAT_ORDER if getattr(args, flag)]
    return bm.encode(fields, tile.numpy("site_status") if st is None else st, tile.numpy("n_alleles"), N)


def test_record_loop_entry_delivers_the_model_bytes():
    """two tiles in flight through vgl_ctx_bcf_keys + vgl_simulate_tile_text_async / vgl_tile_wait give the model's bytes for the same tiles
    (every tag, -doUnobserved 2); the bound follows the encoding; NULL switches back to text"""
    N, S = 300, 64

    def mk():
        return VcfglArgs(seed=21, depth=5, error_rate=0.01, do_unobserved=2, **tt.ALL)
    sim, _, _ = tt.simulate_tile(mk(), N, S)
    ref, _, _ = tt.simulate_tile(mk(), N, S)
    text_bound = int(sim.lib.vgl_ctx_text_bound(sim.ctx, S))
    set_keys(sim)
    assert int(sim.lib.vgl_ctx_text_bound(sim.ctx, S)) < text_bound
    gts = [synth.acgt_sites(S, N, seed=40 + k, missing=0.03) for k in range(2)]
    res = tt.ctx_text(sim, 100, gts)
    fields = ["site_status", "n_alleles"] + [name for _, name, flag in tt.TAGS if getattr(ref.args, flag)]
    for k, ((rc, buf, off, tile), gt) in enumerate(zip(res, gts)):
        assert rc == _abi.VGL_OK, sim.lib.vgl_last_error()
        dtile = ref.new_tile(S, fields=fields, device="cuda:0")
        ref.simulate_device(100 + k * S, torch.from_numpy(gt).cuda(), dtile)
        ref.check()
        want, woff = model_of_tile(ref.args, dtile, N)
        assert np.array_equal(off, woff)
        assert bytes(buf[:len(want)]) == want
        assert (buf[len(want):] == 0x5A).all()                      # only the tile's bytes were copied
        data, doff = bcfenc.encode_records(bcfenc.tile_fields(ref.args, dtile, IDS), dtile["site_status"], dtile["n_alleles"], N)
        assert bytes(data.cpu().numpy()) == want and np.array_equal(doff.cpu().numpy(), woff)
    rc, buf, off, _ = tt.ctx_text(sim, 100, gts[:1], text_cap=1000)[0]
    assert rc == _abi.VGL_E_CAPACITY and int(off[-1]) > 1000 and (buf == 0x5A).all()
    assert sim.lib.vgl_ctx_bcf_keys(sim.ctx, (C.c_int32 * 3)(1, 2, 3), 3) == _abi.VGL_E_ARG
    set_keys(sim, None)
    assert int(sim.lib.vgl_ctx_text_bound(sim.ctx, S)) == text_bound
    rc, buf, off, _ = tt.ctx_text(sim, 100, gts[:1])[0]
    assert rc == _abi.VGL_OK and bytes(buf[:3]) == b"\tDP"
    sim.close()
    ref.close()


def test_deep_rerun_gives_the_same_bytes(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (hooks build): every tile draws deeper than the staging capacity and vgl_tile_wait runs it again,
    encodes and copies again -- the bytes equal those without the hook"""
    N, S = 100, 40
    gts = [synth.acgt_sites(S, N, seed=70 + k, missing=0.03) for k in range(2)]

    def run(hooks):
        args = VcfglArgs(seed=42, depth=20, error_rate=0.01, add_pl=1, add_fmt_ad=1)
        args.rng_mode, args.beta_sampler, args.out_layout = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48, _abi.VGL_LAYOUT_SAMPLE_MAJOR
        sim = Simulator(args, N, max_sites_per_tile=S, hooks=hooks)
        if hooks:
            assert sim.info()["read_cap"] == 8
        set_keys(sim)
        r = tt.ctx_text(sim, 3, gts)
        sim.close()
        return r

    plain = run(False)
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    deep = run(True)
    for (rc0, b0, o0, t0), (rc1, b1, o1, t1) in zip(plain, deep):
        assert rc0 == rc1 == _abi.VGL_OK
        assert np.array_equal(o0, o1) and bytes(b0[:o0[-1]]) == bytes(b1[:o1[-1]]) and o0[-1] > 0
        assert b0[0] == 0x11 and b0[1] == IDS["DP"]                 # typed vectors, not text
        assert int(t1.numpy("fmt_dp").max()) > 8


def test_gvcf_entry_delivers_the_model_bytes_of_records_and_blocks():
    """vgl_ctx_bcf_keys + vgl_simulate_tile_gvcf_async: the records' bytes through record_offsets, the blocks' (PL then DP) behind them
    through block_offsets, both equal to the model over the stateless blocker's outputs; the first / last aggregates stay int32"""
    N, S = 40, 256
    sim = Simulator(tg.sim_args(), N, max_sites_per_tile=S)
    ref = Simulator(tg.sim_args(), N, max_sites_per_tile=S)
    set_keys(sim)
    gts = [tg.hom_ref(S, N, 21), tg.hom_ref(S - 17, N, 22)]
    contigs = [np.zeros(S, np.int32), np.repeat([0, 1], [100, S - 117])]
    pos0s = [np.arange(S) * 1, np.concatenate([np.arange(100) + S, np.arange(S - 117)])]
    dps = [1, 3, 5]
    res = tg.ctx_gvcf(sim, 100, gts, contigs, pos0s, dps)
    s0 = 100
    for (rc, g, keep, tile), gt, contig, pos0 in zip(res, gts, contigs, pos0s):
        assert rc == _abi.VGL_OK, sim.lib.vgl_last_error()
        n = gt.shape[0]
        dtile = tg.simulated(ref, s0, gt)
        c = torch.from_numpy(np.ascontiguousarray(contig, dtype=np.int32)).cuda()
        p = torch.from_numpy(np.ascontiguousarray(pos0, dtype=np.int64)).cuda()
        r = gvcf.blocks_device_raw(dps, dtile["site_status"], dtile["n_alleles_obs"], dtile["n_alleles"], c, p, dtile["fmt_dp"], dtile["pl"].reshape(n, -1))
        assert (g.n_items, g.n_blocks, g.error_site) == (r["n_items"], r["n_blocks"], r["error_site"]) and g.n_blocks > 2
        rwant, roff = model_of_tile(ref.args, dtile, N, st=r["record_status"][:n].cpu().numpy())
        bfields = [(IDS["PL"], r["block_pl"][:n].cpu().numpy().reshape(n, -1), bm.PER_G), (IDS["DP"], r["block_dp"][:n].cpu().numpy().reshape(n, -1), bm.ONE)]
        bwant, boff = bm.encode(bfields, r["block_status"][:n].cpu().numpy(), r["block_n_alleles"][:n].cpu().numpy(), N)
        R = len(rwant)
        assert np.array_equal(keep["roff"], roff) and bytes(keep["text"][:R]) == rwant
        assert np.array_equal(keep["boff"], boff + R) and bytes(keep["text"][R:R + len(bwant)]) == bwant
        assert (keep["text"][R + len(bwant):] == 0x5A).all() and g.text_needed == R + len(bwant)
        assert np.array_equal(keep["fdp"], r["block_dp"][0].cpu().numpy())
        assert np.array_equal(keep["lpl"][: 3 * N], r["block_pl"][g.n_blocks - 1].cpu().numpy()[: 3 * N])
        s0 += n
    (rc, g, keep, _), = tg.ctx_gvcf(sim, 100, gts[:1], contigs[:1], pos0s[:1], dps, text_cap=100)
    assert rc == _abi.VGL_E_CAPACITY and g.text_needed > 100 and (keep["text"] == 0x5A).all()
    sim.close()
    ref.close()


def test_gvcf_deep_rerun_gives_the_same_bytes(monkeypatch):
    N, S = 30, 64
    gts = [tg.hom_ref(S, N, 70 + k) for k in range(2)]
    contigs = [np.zeros(S, np.int32)] * 2
    pos0s = [np.arange(S), np.arange(S) + S]

    def run(hooks):
        sim = Simulator(tg.sim_args(depth=20, error_rate=0.0), N, max_sites_per_tile=S, hooks=hooks)
        if hooks:
            assert sim.info()["read_cap"] == 8
        set_keys(sim)
        r = tg.ctx_gvcf(sim, 3, gts, contigs, pos0s, [10, 12, 14, 16])
        sim.close()
        return r

    plain = run(False)
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    deep = run(True)
    for (rc0, g0, k0, t0), (rc1, g1, k1, t1) in zip(plain, deep):
        assert rc0 == rc1 == _abi.VGL_OK
        assert (g0.n_items, g0.n_blocks, g0.error_site) == (g1.n_items, g1.n_blocks, g1.error_site)
        for k in ("roff", "boff", "fdp", "ldp"):
            assert np.array_equal(k0[k], k1[k]), k
        assert bytes(k0["text"][: k0["boff"][-1]]) == bytes(k1["text"][: k1["boff"][-1]])
        assert int(t1.numpy("fmt_dp").max()) > 8
    assert any(g.n_blocks > 0 for _, g, _, _ in plain)
