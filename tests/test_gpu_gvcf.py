"""The device gVCF blocker (csrc/vgl_gvcf.hip: vgl_gvcf_blocks_device, vgl_simulate_tile_gvcf_async) against the host mirror of the
block machine (vcfgl_amd.gvcf.build): items and aggregates exactly, on synthetic tiles built to reach every rule, on simulated tiles,
through the record-loop entry (with its text) and through the deep-rerun path."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from vcfgl_amd import Simulator, VcfglArgs, _abi, gvcf, vcftext

pytestmark = pytest.mark.gpu
INT32_MISSING = -2147483648


def synthetic(S, N, seed, *, invariant=0.85, skip=0.05, dps=(2, 5, 9), pl_lo=-3, pl_hi=4, dp_hi=12, one_contig=False, step_p=(0.1, 0.8, 0.1)):
    """a tile that reaches every rule: runs of invariant sites, skipped sites inside runs, contig changes, repeated positions and gaps,
    depths crossing the thresholds (r changes, r = 0), negative and missing PL values, ties in PL[1] with different PL[2]"""
    rng = np.random.default_rng(seed)
    st = np.where(rng.random(S) < skip, rng.choice([-3, -4], S), rng.choice([0, 1], S, p=[0.9, 0.1])).astype(np.int32)
    nobs = np.where(rng.random(S) < invariant, 1, rng.integers(2, 5, S)).astype(np.int32)
    na = np.full(S, 2, np.int32)
    contig = np.zeros(S, np.int32) if one_contig else np.cumsum(rng.random(S) < 0.01).astype(np.int32)
    pos0 = np.cumsum(rng.choice([0, 1, 2], S, p=step_p)).astype(np.int64) + 1000
    # depth level per run of sites: every sample near a level, so that the site minimum stays in one range for a while
    level = np.repeat(rng.integers(0, dp_hi, S // 8 + 1), 8)[:S]
    dp = np.clip(level[:, None] + rng.integers(0, 3, (S, N)), 0, None).astype(np.int32)
    G = 15
    pl = np.zeros((S, N * G), np.int32)
    vals = rng.integers(pl_lo, pl_hi, (S, N, 3)).astype(np.int32)
    vals[rng.random((S, N, 3)) < 0.03] = INT32_MISSING
    pl[:, : 3 * N] = vals.reshape(S, 3 * N)
    return dict(st=st, nobs=nobs, na=na, contig=contig, pos0=pos0, dp=dp, pl=pl, dps=list(dps))


def host_items(t):
    S, N = t["dp"].shape
    planes = [np.ascontiguousarray(t["pl"][i, : N * 3].reshape(N, 3).T) for i in range(S)]
    sites = ((i, str(int(t["contig"][i])), int(t["pos0"][i])) for i in range(S))
    return gvcf.build(t["dps"], sites, t["st"], t["nobs"], t["na"], t["dp"], planes)


def device_items(t, raw=False):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (t["dps"], dev(t["st"]), dev(t["nobs"]), dev(t["na"]), dev(t["contig"]), dev(t["pos0"]), dev(t["dp"]), dev(t["pl"]))
    return gvcf.blocks_device_raw(*args) if raw else gvcf.blocks_device(*args)


def same_items(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0]
        if x[0] == "rec":
            assert x[1] == y[1]
        else:
            assert x[1].same(y[1]), (x[1], y[1])


@pytest.mark.parametrize("N", [1, 3, 64, 65, 1000])
@pytest.mark.parametrize("seed", [1, 2])
def test_synthetic_tiles_equal_the_host_machine(N, seed):
    S = 3000 if N < 1000 else 600
    t = synthetic(S, N, seed * 100 + N)
    want = host_items(t)
    got = device_items(t)
    same_items(got, want)
    kinds = [k for k, _ in want]
    assert "rec" in kinds and "block" in kinds
    assert any(b.end > b.start for k, b in want if k == "block") and any(b.end == b.start for k, b in want if k == "block")


def test_few_sites_and_one_site_blocks():
    for S in (1, 2, 5, 33, 1025):
        for seed in range(3):
            t = synthetic(S, 3, 5000 + S * 10 + seed, dps=(1, 2, 3, 4, 5, 6, 7, 8), dp_hi=9)
            same_items(device_items(t), host_items(t))


def test_one_block_covers_a_whole_tile():
    S, N = 65536, 1
    t = synthetic(S, N, 9, invariant=1.0, skip=0.0, dps=(1,), dp_hi=1, one_contig=True, step_p=(0.05, 0.95, 0.0))
    t["dp"][:] = 5
    t["st"][0] = 0
    want = host_items(t)
    assert len(want) == 1 and want[0][0] == "block"
    same_items(device_items(t), want)
    t2 = dict(t, dp=np.full((S, 3), 5, np.int32), pl=np.tile(t["pl"][:, :1], (1, 45)))
    same_items(device_items(t2), host_items(t2))


def test_ties_in_pl1_pick_the_smaller_pl2():
    S, N = 4, 2
    t = synthetic(S, N, 3, invariant=1.0, skip=0.0, one_contig=True, step_p=(0.0, 1.0, 0.0))
    t["dp"][:] = 6
    t["pl"][:] = 0
    for i, (p1, p2) in enumerate([(5, 9), (5, 3), (5, 7), (6, -1)]):
        t["pl"][i, :6] = [i, p1, p2, i, p1 - 10, p2]
    got = device_items(t)
    assert len(got) == 1
    b = got[0][1]
    assert b.pl[:, 0].tolist() == [0, 5, 3] and b.pl[:, 1].tolist() == [0, -5, 3]
    same_items(got, host_items(t))


def test_five_allele_founder_alone_and_joined():
    S, N = 6, 3
    t = synthetic(S, N, 4, invariant=1.0, skip=0.0, one_contig=True, step_p=(0.0, 1.0, 0.0))
    t["dp"][:] = 6
    t["dp"][1] = 0                                                       # site 1 is a record (r = 0): site 2 founds a lone block
    t["dp"][3] = 0
    t["na"][2] = 5
    t["pl"][2, : 15 * N] = np.arange(15 * N)
    got = device_items(t)
    blocks = [b for k, b in got if k == "block"]
    lone = [b for b in blocks if b.founder == 2][0]
    assert lone.start == lone.end and lone.pl.shape == (15, N)
    assert np.array_equal(lone.pl, np.arange(15 * N).reshape(N, 15).T)
    # joined by a member: the error site is reported (the host's "Unexpected number of PL values"); a 5-allele member also
    t["dp"][3] = 6
    r = device_items(t, raw=True)
    assert r["error_site"] == 3
    with pytest.raises(gvcf.GvcfError) as e:
        device_items(t)
    assert e.value.site == 3 and e.value.n_values == 3 * N
    t["na"][2] = 2
    t["na"][4] = 5
    assert device_items(t, raw=True)["error_site"] == 4


def test_two_runs_give_identical_bytes():
    t = synthetic(5000, 65, 77)
    a, b = device_items(t, raw=True), device_items(t, raw=True)
    assert a["n_items"] == b["n_items"] and np.array_equal(a["items"], b["items"])
    nb = a["n_blocks"]
    for k in ("block_dp", "block_pl", "block_n_alleles", "block_status", "record_status"):
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        if k in ("block_dp", "block_pl"):
            x, y = x[:nb, : 3 * 65], y[:nb, : 3 * 65]                   # (a slab behind the block's own values is not written)
        assert np.array_equal(x, y), k


def sim_args(**kw):
    args = VcfglArgs(seed=kw.pop("seed", 31), depth=kw.pop("depth", 4), error_rate=kw.pop("error_rate", 0.002), do_unobserved=2, add_pl=1,
                     do_gvcf=1, **kw)
    args.rng_mode, args.beta_sampler, args.out_layout = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48, _abi.VGL_LAYOUT_SAMPLE_MAJOR
    return args


def simulated(sim, site0, gt):
    S = gt.shape[0]
    tile = sim.new_tile(S, fields=["site_status", "n_alleles", "n_alleles_obs", "fmt_dp", "pl", "gl"], device="cuda:0")
    sim.simulate_device(site0, torch.from_numpy(gt).cuda(), tile)
    sim.check()
    torch.cuda.synchronize()
    return tile


def hom_ref(S, N, seed):
    gt = synth.acgt_sites(S, N, seed=seed, missing=0.0)
    ref = gt[:, :1] & 0x0F
    return np.ascontiguousarray((ref | (ref << 4)).repeat(N, axis=1).astype(np.uint8))


@pytest.mark.parametrize("N", [1, 5, 130])
def test_simulated_tiles_equal_the_host_machine(N):
    S = 512
    sim = Simulator(sim_args(), N, max_sites_per_tile=S)
    gt = hom_ref(S, N, 11)
    tile = simulated(sim, 7, gt)
    contig = torch.zeros(S, dtype=torch.int32, device="cuda")
    pos0 = torch.arange(S, dtype=torch.int64, device="cuda") * 1 + 50
    dps = [1, 3, 5, 8]
    pl = tile["pl"].reshape(S, -1)
    got = gvcf.blocks_device(dps, tile["site_status"], tile["n_alleles_obs"], tile["n_alleles"], contig, pos0, tile["fmt_dp"], pl, site0=7)
    G = tile.G
    t = dict(st=tile.numpy("site_status"), nobs=tile.numpy("n_alleles_obs"), na=tile.numpy("n_alleles"), contig=contig.cpu().numpy(),
             pos0=pos0.cpu().numpy(), dp=tile.numpy("fmt_dp"), pl=pl.cpu().numpy(), dps=dps)
    want = [(k, v + 7) if k == "rec" else (k, v) for k, v in host_items(t)]
    for k, v in want:
        if k == "block":
            v.founder += 7
    same_items(got, want)
    assert sum(1 for k, _ in want if k == "block") > 3
    sim.close()


def ctx_gvcf(sim, site0, gts, contigs, pos0s, dps, text_cap=None):
    """vgl_simulate_tile_gvcf_async for consecutive tiles, all in flight before the first wait"""
    lib = sim.lib
    S = sim.max_sites_per_tile
    cap = int(lib.vgl_ctx_gvcf_text_bound(sim.ctx, S))
    N, G = sim.n_samples, sim.G
    subs = []
    dps_a = (C.c_int32 * len(dps))(*dps)
    s0 = site0
    for gt, contig, pos0 in zip(gts, contigs, pos0s):
        n = gt.shape[0]
        tile = sim.new_tile(n, fields=["site_status", "n_alleles", "n_alleles_obs", "fmt_dp"])
        keep = dict(text=np.full(cap, 0x5A, np.uint8), roff=np.zeros(n + 1, np.int64), boff=np.zeros(n + 1, np.int64),
                    items=np.zeros(n * 8, np.int32), fdp=np.zeros(N, np.int32), ldp=np.zeros(N, np.int32),
                    fpl=np.zeros(N * G, np.int32), lpl=np.zeros(N * G, np.int32), gt=np.ascontiguousarray(gt),
                    contig=np.ascontiguousarray(contig, dtype=np.int32), pos0=np.ascontiguousarray(pos0, dtype=np.int64))
        g = _abi.GvcfTile(keep["items"].ctypes.data, keep["text"].ctypes.data, cap if text_cap is None else text_cap, keep["roff"].ctypes.data,
                          keep["boff"].ctypes.data, keep["fdp"].ctypes.data, keep["fpl"].ctypes.data, keep["ldp"].ctypes.data,
                          keep["lpl"].ctypes.data, 0, 0, 0, 0, 0)
        t = C.c_int32()
        sim._check(lib.vgl_simulate_tile_gvcf_async(sim.ctx, s0, n, keep["gt"].ctypes.data, keep["contig"].ctypes.data, keep["pos0"].ctypes.data,
                                                     dps_a, len(dps), tile.byref(), C.byref(g), C.byref(t)))
        subs.append((t.value, g, keep, tile))
        s0 += n
    out = []
    for t, g, keep, tile in subs:
        rc = lib.vgl_tile_wait(sim.ctx, t)
        out.append((rc, g, keep, tile))
    return out


def stateless(sim, site0, gt, contig, pos0, dps):
    """the tile through the device path and the stateless entries: (raw blocker outputs, record text, record offsets, block text,
    block offsets)"""
    S, N = gt.shape
    tile = simulated(sim, site0, gt)
    c = torch.from_numpy(np.ascontiguousarray(contig, dtype=np.int32)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(pos0, dtype=np.int64)).cuda()
    pl = tile["pl"].reshape(S, -1)
    r = gvcf.blocks_device_raw(dps, tile["site_status"], tile["n_alleles_obs"], tile["n_alleles"], c, p, tile["fmt_dp"], pl)
    rtext, roff = vcftext.format_columns(vcftext.tile_fields(sim.args, tile), r["record_status"][:S], tile["n_alleles"], N)
    bfields = [("PL", r["block_pl"][:S], vcftext.PER_G), ("DP", r["block_dp"][:S], vcftext.ONE)]
    btext, boff = vcftext.format_columns(bfields, r["block_status"][:S], r["block_n_alleles"][:S], N)
    return r, bytes(rtext.cpu().numpy()), roff.cpu().numpy(), bytes(btext.cpu().numpy()), boff.cpu().numpy(), tile


def check_against_stateless(sim, ref, site0, gts, contigs, pos0s, dps):
    res = ctx_gvcf(sim, site0, gts, contigs, pos0s, dps)
    s0 = site0
    for (rc, g, keep, tile), gt, contig, pos0 in zip(res, gts, contigs, pos0s):
        assert rc == _abi.VGL_OK, sim.lib.vgl_last_error()
        n, N = gt.shape
        r, rtext, roff, btext, boff, dtile = stateless(ref, s0, gt, contig, pos0, dps)
        assert g.n_items == r["n_items"] and g.n_blocks == r["n_blocks"] and g.error_site == r["error_site"]
        assert np.array_equal(keep["items"][: g.n_items * 8].reshape(-1, 8), np.array(r["items"].tolist(), dtype=np.int32).reshape(-1, 8))
        assert np.array_equal(keep["roff"], roff)
        R = int(roff[-1])
        assert bytes(keep["text"][:R]) == rtext
        assert np.array_equal(keep["boff"], boff + R)
        assert bytes(keep["text"][R:R + int(boff[-1])]) == btext
        assert (keep["text"][R + int(boff[-1]):] == 0x5A).all()
        nb = g.n_blocks
        if nb:
            assert np.array_equal(keep["fdp"], r["block_dp"][0].cpu().numpy())
            assert np.array_equal(keep["ldp"], r["block_dp"][nb - 1].cpu().numpy())
            assert np.array_equal(keep["fpl"][: 3 * N], r["block_pl"][0].cpu().numpy()[: 3 * N])
            assert np.array_equal(keep["lpl"][: 3 * N], r["block_pl"][nb - 1].cpu().numpy()[: 3 * N])
        for f in ("site_status", "n_alleles", "n_alleles_obs", "fmt_dp"):
            assert np.array_equal(tile.numpy(f), dtile.numpy(f)), f
        s0 += n
    return res


def test_record_loop_entry_equals_the_stateless_entry():
    N, S = 40, 256
    sim = Simulator(sim_args(), N, max_sites_per_tile=S)
    ref = Simulator(sim_args(), N, max_sites_per_tile=S)
    gts = [hom_ref(S, N, 21), hom_ref(S - 17, N, 22)]
    contigs = [np.zeros(S, np.int32), np.repeat([0, 1], [100, S - 117])]
    pos0s = [np.arange(S) * 1, np.concatenate([np.arange(100) + S, np.arange(S - 117)])]
    res = check_against_stateless(sim, ref, 100, gts, contigs, pos0s, [1, 3, 5])
    assert all(g.n_blocks > 2 for _, g, _, _ in res)
    # a text larger than text_cap: VGL_E_CAPACITY, the size needed, nothing written
    (rc, g, keep, _), = ctx_gvcf(sim, 100, gts[:1], contigs[:1], pos0s[:1], [1, 3, 5], text_cap=100)
    assert rc == _abi.VGL_E_CAPACITY and g.text_needed > 100 and (keep["text"] == 0x5A).all()
    sim.close()
    ref.close()


def test_deep_rerun_gives_the_same_items_and_text(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (hooks build): every tile draws deeper than the staging capacity and vgl_tile_wait runs it again,
    blocks and formats it again -- the items and text equal those without the hook"""
    N, S = 30, 64
    gts = [hom_ref(S, N, 70 + k) for k in range(2)]
    contigs = [np.zeros(S, np.int32)] * 2
    pos0s = [np.arange(S), np.arange(S) + S]

    def run(hooks):
        sim = Simulator(sim_args(depth=20, error_rate=0.0), N, max_sites_per_tile=S, hooks=hooks)
        if hooks:
            assert sim.info()["read_cap"] == 8
        r = ctx_gvcf(sim, 3, gts, contigs, pos0s, [10, 12, 14, 16])
        sim.close()
        return r

    plain = run(False)
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    deep = run(True)
    for (rc0, g0, k0, t0), (rc1, g1, k1, t1) in zip(plain, deep):
        assert rc0 == rc1 == _abi.VGL_OK
        assert (g0.n_items, g0.n_blocks, g0.error_site) == (g1.n_items, g1.n_blocks, g1.error_site)
        assert np.array_equal(k0["items"][: g0.n_items * 8], k1["items"][: g1.n_items * 8])
        for k in ("roff", "boff", "fdp", "ldp"):
            assert np.array_equal(k0[k], k1[k]), k
        assert bytes(k0["text"][: k0["boff"][-1]]) == bytes(k1["text"][: k1["boff"][-1]])
        assert int(t1.numpy("fmt_dp").max()) > 8
    assert any(g.n_blocks > 0 for _, g, _, _ in plain)
