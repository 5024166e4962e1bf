"""The discordance tally on the device (vgl_disc.hip) against the model (tests/disc_model.py): the kernel alone on synthetic tiles,
the width of its counters, the context path behind every kind of likelihood kernel, and the host program's --gt-discordance."""
import os
import subprocess

import numpy as np
import pytest

import disc_model as dm
import synth
from vcfgl_amd import Simulator, VcfglArgs, _abi
from vcfgl_amd.discordance import format_table, new_table, tally_into
from vcfgl_amd.tile import Tile
from vcfgl_amd.vcfio import read_vcf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data")
G = 15


def synthetic_tile(rng, S, N):
    """arrays in which every branch of the tally occurs: 1 .. 5 alleles in any order (the unobserved allele in any position, the first
    included), PL ties at 0, vectors of zeros, values of 255 and (int32) beyond, samples without reads, missing true alleles, true
    heterozygotes in both nibble orders, skipped sites and sites without reads"""
    status = rng.choice(np.array([0, 0, 0, 0, 1, -3, -4], dtype=np.int32), size=S)
    nA = rng.integers(1, 6, size=S).astype(np.int32)
    a2b = np.full((S, 5), -1, dtype=np.int8)
    for i in range(S):
        a2b[i, :nA[i]] = rng.permutation(5)[:nA[i]]
    dp = rng.integers(1, 40, size=(S, N)).astype(np.int32)
    dp[rng.random((S, N)) < 0.15] = 0
    dp[status == 1] = 0
    P = rng.integers(0, 90, size=(S, N, G)).astype(np.int32)
    kind = rng.integers(0, 6, size=(S, N))
    zero_at = rng.integers(0, G, size=(S, N, 2))
    si, ni = np.meshgrid(np.arange(S), np.arange(N), indexing="ij")
    P[si, ni, zero_at[:, :, 0] % np.maximum(nA * (nA + 1) // 2, 1)[:, None]] = 0               # one zero among the site's genotypes
    two = kind == 1
    P[si[two], ni[two], (zero_at[:, :, 1] % np.maximum(nA * (nA + 1) // 2, 1)[:, None])[two]] = 0     # a tie at 0
    P[kind == 2] = 0                                                                          # every PL 0
    big = (kind == 3)[:, :, None] & (rng.random((S, N, G)) < 0.5)
    P[big] = 255                                                                              # capped values
    huge = (kind == 4)[:, :, None] & (rng.random((S, N, G)) < 0.4) & (P != 0)
    P[huge] = rng.integers(256, 5000, size=int(huge.sum()))                                   # int32 only: beyond the cap
    nib = rng.integers(0, 4, size=(S, N, 2)).astype(np.uint8)
    nib[rng.random((S, N, 2)) < 0.04] = 0xF
    gt = (nib[:, :, 0] | (nib[:, :, 1] << 4)).astype(np.uint8)
    return status, nA, a2b, dp, P, gt


def lay_out(P, nA, dp, layout, u8, rng):
    """[S][N][G] logical values -> the library's [S][G][N] buffer in `layout`; what a site does not own is the missing value
    (planes) or noise (sample-major: the kernels leave it unwritten)"""
    S, N, _ = P.shape
    miss = 255 if u8 else dm.INT32_MISSING
    V = np.where(dp[:, :, None] == 0, miss, np.minimum(P, 255) if u8 else P)
    if layout == dm.PLANES:
        buf = np.full((S, G, N), miss, dtype=np.int64)
        for i in range(S):
            nG = nA[i] * (nA[i] + 1) // 2
            buf[i, :nG, :] = V[i, :, :nG].T
    else:
        buf = rng.integers(0, 256, size=(S, G, N)).astype(np.int64)
        for i in range(S):
            nG = nA[i] * (nA[i] + 1) // 2
            buf[i].reshape(-1)[:N * nG] = V[i, :, :nG].reshape(-1)
    return buf.astype(np.uint8 if u8 else np.int32)


@pytest.mark.parametrize("S", [1, 7, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_kernel_alone_equals_the_model(N, S):
    import torch
    rng = np.random.default_rng(1000 * N + S)
    status, nA, a2b, dp, P, gt = synthetic_tile(rng, S, N)
    g = torch.from_numpy(gt).to("cuda:0")
    want = None
    for layout in (dm.PLANES, dm.SAMPLE_MAJOR):
        for u8 in (True, False):
            buf = lay_out(P, nA, dp, layout, u8, rng)
            name = "pl_u8" if u8 else "pl"
            tile = Tile(S, N, 5, G, fields=["fmt_dp", name], device="cuda:0")
            for k, v in (("site_status", status), ("n_alleles", nA), ("alleles2acgt", a2b), ("fmt_dp", dp), (name, buf)):
                tile.arrays[k].copy_(torch.from_numpy(v))
            model = dm.tally(status, nA, a2b, dp, buf, gt, layout=layout)
            if want is None:
                want = model
                c, mis, sites = dm.views(want, N)
                if S == 300 and N >= 63:                        # the generator reaches every cell, missing calls and both kinds of site
                    assert (c.sum(axis=(0, 2)) > 0).all() and mis.sum() > 0 and sites.min() > 0
                    assert c[:, :, 127].sum() > 0 and c[:, :, 1:127].sum() > 0
            assert np.array_equal(model, want), "the model gives one table for both layouts and both PL forms"
            table = new_table(N, "cuda:0")
            tally_into(tile, g, table, layout=layout)
            got = table.cpu().numpy()
            assert np.array_equal(got, want), (layout, u8, int(np.abs(got - want).sum()))
            tally_into(tile, g, table, layout=layout)            # a second call adds
            assert np.array_equal(table.cpu().numpy(), 2 * want), (layout, u8)
    torch.cuda.synchronize()


def test_counts_beyond_sixteen_bits():
    """N = 3, 70 000 sites in tiles of 4096 (18 tiles), -e 0 -d 30: equal to the model applied to the same tiles' arrays.  Without
    errors nearly every call has GQ 127, so one bin per sample takes nearly all 70 000 counts -- more than a 16-bit counter holds"""
    depth = 30
    N, S, TS = 3, 70000, 4096
    args = VcfglArgs(seed=7, depth=depth, error_rate=0.0, add_pl=1)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    gt = np.zeros((S, N), dtype=np.uint8)
    gt[:, 1] = 0x11
    gt[:, 2] = 0x10
    sim = Simulator(args, N, max_sites_per_tile=TS)
    sim.discordance(1)
    want = np.zeros(dm.table_len(N), dtype=np.int64)
    for t0 in range(0, S, TS):
        tile = sim.simulate(t0, gt[t0:t0 + TS], fields=["fmt_dp", "pl_u8"])
        dm.tally(tile.numpy("site_status"), tile.numpy("n_alleles"), tile.numpy("alleles2acgt"), tile.numpy("fmt_dp"), tile.numpy("pl_u8"),
                 gt[t0:t0 + TS], table=want)
    got = sim.discordance_table()
    sim.close()
    cell, mis, sites = dm.views(got, N)
    print("largest bin", int(cell.max()), "at depth", depth)
    assert np.array_equal(got, want)
    assert sites[0] + sites[1] == S and cell.sum() + mis.sum() == sites[0] * N
    assert cell[:, :, 127].max() > 65536


CASES = [
    ("fused", dict(depth=5.0, error_rate=0.01)),
    ("three_kernels", dict(depth=20.0, error_rate=0.01)),
    ("gl1", dict(depth=9.0, error_rate=0.02, gl_model=1)),
    ("precise", dict(depth=14.0, error_rate=0.03, error_qs=2, beta_variance=1e-5, precise_gl=1)),
    ("perread", dict(depth=20.0, error_rate=0.01, error_qs=2, beta_variance=1e-5)),
    ("alltags", dict(depth=10.0, error_rate=0.05, add_gp=1, add_qs=1, add_i16=1, add_fmt_ad=1, add_fmt_adf=1, add_fmt_adr=1, add_info_ad=1)),
    ("shallow", dict(depth=0.5, error_rate=0.01)),
    ("rm", dict(depth=1.0, error_rate=0.01, rm_invar_sites=4, rm_empty_sites=1)),
] + [("du%d" % du, dict(depth=6.0, error_rate=0.2, do_unobserved=du)) for du in range(6)]


@pytest.mark.parametrize("N", [1, 65, 1025])
@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_context_tallies_every_tile(name, kw, N):
    """Simulator.discordance(1): the table equals the model applied to the PL / DP / allele arrays the same run returned, whether or
    not the caller asks for PL, in both layouts; every returned array equals that of a run with the tally off"""
    S = 150 if N < 1000 else 40
    gt = synth.acgt_sites(S, N, seed=N + len(name), missing=0.03)
    for layout in (_abi.VGL_LAYOUT_PLANES, _abi.VGL_LAYOUT_SAMPLE_MAJOR):
        args = VcfglArgs(seed=42, add_pl=1, **kw)
        args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
        args.out_layout = layout
        off = Simulator(args, N, max_sites_per_tile=S)
        if name == "fused" and N == 1025:
            assert off.info()["fused"] == 1
        base = off.simulate(3, gt)
        off.close()
        want = dm.tally(base.numpy("site_status"), base.numpy("n_alleles"), base.numpy("alleles2acgt"), base.numpy("fmt_dp"), base.numpy("pl"),
                        gt, layout=layout)
        cell, mis, sites = dm.views(want, N)
        if name == "shallow":
            assert mis.sum() > cell.sum() > 0                       # many calls are missing
        if name == "rm" and N == 1:
            assert sites[1] > 0                                     # (a site of one sample is often empty or invariable)
        on = Simulator(args, N, max_sites_per_tile=S)
        on.discordance(1)
        full = on.simulate(3, gt)                                   # PL and DP among the outputs
        assert np.array_equal(on.discordance_table(reset=True), want), (name, layout, "with PL")
        lean = on.simulate(3, gt, fields=["gl"])                    # neither: the context keeps them on the device
        assert np.array_equal(on.discordance_table(), want), (name, layout, "without PL")
        narrow = on.simulate(3, gt, fields=["fmt_dp", "pl_u8"])
        assert np.array_equal(on.discordance_table(reset=True), 2 * want), (name, layout, "pl_u8")
        on.discordance(0)
        on.simulate(3, gt, fields=["gl"])
        assert not on.discordance_table().any()                     # switched off: nothing is counted
        on.close()
        for f in base.arrays:
            assert np.array_equal(base.numpy(f).view(np.uint8), full.numpy(f).view(np.uint8)), (name, layout, f)
        assert np.array_equal(base.numpy("gl").view(np.uint32), lean.numpy("gl").view(np.uint32))
        assert np.array_equal(base.numpy("fmt_dp"), narrow.numpy("fmt_dp"))


def test_serial_mode_tiles_and_the_device_entry_point():
    import torch
    N, S, TS = 70, 90, 32
    gt = synth.acgt_sites(S, N, seed=5, missing=0.03)
    args = VcfglArgs(seed=3, depth=4.0, error_rate=0.05, add_pl=1)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_SERIAL, _abi.VGL_BETA_STD
    sim = Simulator(args, N, max_sites_per_tile=TS)
    sim.discordance(1)
    want = np.zeros(dm.table_len(N), dtype=np.int64)
    for t0 in range(0, S, TS):
        t = sim.simulate(t0, gt[t0:t0 + TS])
        dm.tally(t.numpy("site_status"), t.numpy("n_alleles"), t.numpy("alleles2acgt"), t.numpy("fmt_dp"), t.numpy("pl"), gt[t0:t0 + TS], table=want)
    assert np.array_equal(sim.discordance_table(), want)
    sim.close()
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    sim = Simulator(args, N, max_sites_per_tile=S)
    sim.discordance(1)
    tile = sim.new_tile(S, fields=["gl"], device="cuda:0")
    sim.simulate_device(0, torch.from_numpy(gt).to("cuda:0"), tile)
    sim.check()
    got = sim.discordance_table()
    ref = sim.simulate(0, gt)
    sim.close()
    assert np.array_equal(got, dm.tally(ref.numpy("site_status"), ref.numpy("n_alleles"), ref.numpy("alleles2acgt"), ref.numpy("fmt_dp"),
                                        ref.numpy("pl"), gt))


def test_a_tile_that_is_run_again_is_counted_once(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (the hooks build): every tile draws deeper than the staging capacity and is run again on the
    sibling context, in sub-tiles; the first run is not counted"""
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    N, S = 100, 2500
    args = VcfglArgs(seed=42, depth=20, error_rate=0.01, add_pl=1)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    gt = synth.acgt_sites(S, N, seed=S, missing=0.03)
    sim = Simulator(args, N, max_sites_per_tile=S, hooks=True)
    assert sim.info()["read_cap"] == 8
    sim.discordance(1)
    t = sim.simulate(3, gt)
    got = sim.discordance_table()
    sim.close()
    want = dm.tally(t.numpy("site_status"), t.numpy("n_alleles"), t.numpy("alleles2acgt"), t.numpy("fmt_dp"), t.numpy("pl"), gt)
    assert np.array_equal(got, want)


def _run(out, inp, *flags):
    r = subprocess.run([BIN, "-i", os.path.join(DATA, inp), "-o", out, "--seed", "42", "-e", "0.05", "--tile-sites", "7", "-addPL", "1"] + list(flags),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    path = out + ".discordance.tsv"
    return open(path).read() if os.path.exists(path) else None


def _body(path):
    return [ln for ln in open(path) if not ln.startswith("##source=")]


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("inp,src", [("data3.vcf", ["-explode", "1", "-d", "3"]), ("data5_acgt_multiallelic.vcf", ["--source", "1", "-d", "2"]),
                                     ("data3.vcf", ["-explode", "1", "-d", "0.7", "--rm-empty-sites", "1", "--rm-invar-sites", "4"])])
def test_cli_discordance_file(inp, src, tmp_path):
    o = lambda k: str(tmp_path / k)
    base = ["-O", "v", "-printTruth", "1", "--gt-discordance", "1"] + src
    tsv0 = _run(o("m0"), inp, *base)
    truth, recs = read_vcf(o("m0") + ".truth.vcf"), read_vcf(o("m0") + ".vcf")
    want = dm.tally_records(truth, recs)
    assert dm.views(want, len(truth.samples))[0].sum() > 0
    assert tsv0 == format_table(want, truth.samples, 0)
    for mode in (3, 4, 5, 6):
        assert _run(o("m%d" % mode), inp, "--discordance-gq", str(mode), *base) == format_table(want, truth.samples, mode), mode
    # the same table whatever writes the records, on one device or two contexts, and with no records at all
    assert _run(o("dev2"), inp, "--devices", "0,0", *base) == tsv0
    assert _run(o("bcf"), inp, "-O", "b", "--device-bcf", "1", "--device-stream", "1", "--gt-discordance", "1", *src) == tsv0
    assert _run(o("txt"), inp, "-O", "z", "--device-text", "1", "--gt-discordance", "1", *src) == tsv0
    assert _run(o("nopl"), inp, "-O", "u", "-addPL", "0", "--gt-discordance", "1", *src) == tsv0
    assert _run(o("pile"), inp, "-O", "v", "-printPileup", "1", "--device-pileup", "1", "--gt-discordance", "1", *src) == tsv0
    assert _run(o("norec"), inp, "--records", "0", "--gt-discordance", "1", *src) == tsv0
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("norec") and f not in ("norec.arg", "norec.discordance.tsv")]
    # the records are those of a run without the tally
    assert _run(o("off"), inp, "-O", "v", "-printTruth", "1", *src) is None
    assert _body(o("off") + ".vcf") == _body(o("m0") + ".vcf") and _body(o("off") + ".truth.vcf") == _body(o("m0") + ".truth.vcf")
    # the reference's draw order: against its own records
    tsv1 = _run(o("serial"), inp, "--rng-mode", "1", *base)
    assert tsv1 == format_table(dm.tally_records(read_vcf(o("serial") + ".truth.vcf"), read_vcf(o("serial") + ".vcf")), truth.samples, 0)


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_cli_discordance_with_gvcf_blocks(tmp_path):
    o = lambda k: str(tmp_path / k)
    flags = ["-explode", "1", "-d", "3", "-doGVCF", "1", "--gvcf-dps", "1,5,10", "--gt-discordance", "1", "--discordance-gq", "6"]
    plain = _run(o("plain"), "data3.vcf", "-O", "v", "-explode", "1", "-d", "3", "--gt-discordance", "1", "--discordance-gq", "6")
    assert _run(o("host"), "data3.vcf", "-O", "v", *flags) == plain
    assert _run(o("dev"), "data3.vcf", "-O", "v", "--device-gvcf", "1", *flags) == plain
