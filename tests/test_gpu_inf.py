"""vgl_inf_fill_device and vgl_ctx_true_values on the device, bit for bit against the numpy model of the reference's
simulate_record_true_values (tests/inf_model.py): every per-site array and every GL / GP / PL / one-byte PL value, in both layouts,
for every -doUnobserved and every subset of the outputs, at the sample counts where k_inf_site changes its sub-group (1, 2, 3, 63,
64, 65) and k_inf_fill takes more than one workgroup per site (130 x 15 sample-major values), with guard regions around every array.
Then the context switch: through vgl_simulate_tile and vgl_simulate_tile_device, a tile split anywhere, the refusals, and simulated
tiles around a true-value one."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import inf_model as im
from vcfgl_amd import Simulator, VcfglArgs, VglError, _abi, truevals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                                                        # guard elements on either side of every array
SENT = 0xA5                                                     # every byte of a guard and of an array before the call
OUTS = ("gl", "gp", "pl", "pl_u8")
TORCH = {"gl": torch.float32, "gp": torch.float32, "pl": torch.int32, "pl_u8": torch.uint8, "site_status": torch.int32, "n_alleles": torch.int32,
         "n_alleles_obs": torch.int32, "alleles2acgt": torch.int8}


def site_from_counts(counts, N, rng):
    """(tiny N: a pattern that does not fit the 2 N alleles there are is cut or padded with its first base)"""
    alleles = np.repeat(np.arange(4), np.maximum(counts, 0))[:2 * N]
    alleles = np.concatenate([alleles, np.full(2 * N - alleles.size, int(np.argmax(counts)))])
    rng.shuffle(alleles)                                        # (pairs in either order: hets with the rarer base in the low and in the high nibble)
    return (alleles[0::2] | (alleles[1::2] << 4)).astype(np.uint8)


def make_gt(S, N, seed):
    """S sites x N samples: one allele only, 2, 3 and 4 observed alleles, two-, three- and four-way ties, the rest random -- each with
    the bases permuted, so that a tie is decided among every set of bases"""
    rng = np.random.default_rng(seed)
    M = 2 * N
    k3, k4 = (M - 1) // 3, M // 4                                # ([r, k3, k3, k3] with 0 < r <= 3: such as [1, 2, 2, 2])
    patterns = [[M, 0, 0, 0], [M - 1, 1, 0, 0], [M - 2, 1, 1, 0], [M - 3, 1, 1, 1], [M // 2, M // 2, 0, 0], [M - 3 * k3, k3, k3, k3],
                [k4, k4, k4, M - 3 * k4], [M - 2 * (M // 3), M // 3, M // 3, 0]]
    gt, counts = np.zeros((S, N), np.uint8), []
    for i in range(S):
        c = patterns[i % 10] if i % 10 < len(patterns) else list(rng.multinomial(M, rng.dirichlet(np.ones(4))))
        c = [int(c[j]) for j in rng.permutation(4)]
        gt[i] = site_from_counts(c, N, rng)
        counts.append([int(np.sum((gt[i] & 0xF) == b) + np.sum((gt[i] >> 4) == b)) for b in range(4)])
    return gt, counts


def guarded(n, dtype):
    """a device array of n elements with PAD guard elements on either side, every byte SENT; returns (whole, interior view)"""
    item = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full(((n + 2 * PAD) * item,), SENT, dtype=torch.uint8, device=DEV).view(dtype)
    return whole, whole[PAD:PAD + n]


def as_bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def run_fill(gt, d, layout, subset):
    S, N = gt.shape
    G = im.max_genotypes(d)
    arrays = {k: guarded(S * (5 if k == "alleles2acgt" else 1), TORCH[k]) for k in ("site_status", "n_alleles", "n_alleles_obs", "alleles2acgt")}
    arrays.update({k: guarded(S * G * N, TORCH[k]) for k in subset})
    gt_t = torch.from_numpy(gt).to(DEV)
    bad_w, bad = guarded(1, torch.int32)
    bad.fill_(im.NO_SITE)
    ws_w, ws = guarded(truevals.workspace_bytes(N, S), torch.uint8)
    truevals.fill_into(gt_t, *(arrays[k][1] for k in ("site_status", "n_alleles", "n_alleles_obs", "alleles2acgt")), do_unobserved=d, bad_site=bad, workspace=ws,
                       layout=layout, **{k: arrays[k][1] for k in subset})
    torch.cuda.synchronize()
    for k, (whole, view) in list(arrays.items()) + [("bad_site", (bad_w, bad)), ("workspace", (ws_w, ws))]:
        b, item = as_bytes(whole), whole.element_size()
        assert (b[:PAD * item] == SENT).all() and (b[-PAD * item:] == SENT).all(), ("guard of " + k, S, N, d, layout, subset)
    return {k: v[1].cpu().numpy() for k, v in arrays.items()}, int(bad.item())


def check_against_model(got, bad_got, want, subset, ctx=()):
    good = np.ones(len(want["n_alleles"]), bool)
    good[im.bad_sites(want["gt"])] = False
    assert bad_got == want["bad_site"], ctx
    for k in ("site_status", "n_alleles", "n_alleles_obs", "alleles2acgt"):
        assert np.array_equal(got[k].reshape(len(good), -1)[good], want[k].reshape(len(good), -1)[good]), (k,) + tuple(ctx)
    for k in subset:
        g = got[k].reshape(want[k].shape)
        g = g.view(np.uint32) if k in ("gl", "gp") else g
        w, mask = want[k], want["written"]
        assert np.array_equal(g[mask], w[mask]), (k,) + tuple(ctx)
        # what the call does not define it does not touch: sample-major, behind N nG of a good site's slab
        rest = ~mask & good[:, None]
        sent = np.frombuffer(bytes([SENT]) * g.dtype.itemsize, g.dtype)[0]
        assert (g[rest] == sent).all(), (k, "written behind the record's array") + tuple(ctx)


def model(gt, d, layout):
    m = im.fill(gt, d, layout)
    m["gt"] = gt
    return m


SUBSETS = [tuple(k for k, on in zip(OUTS, bits) if on) for bits in itertools.product((0, 1), repeat=4)]


@pytest.mark.parametrize("S", [1, 67])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 130])
def test_fill_equals_the_model(N, S):
    gt, counts = make_gt(S, N, seed=1000 * N + S)
    if S == 67 and N >= 63:                                     # the sites the shapes are chosen for are all there
        ties = lambda c, n: sorted(c)[-n:] == [max(c)] * n and (n == 4 or sorted(c)[-n - 1] < max(c))
        assert {sum(1 for x in c if x) for c in counts} == {1, 2, 3, 4}
        assert all(any(ties(c, n) for c in counts) for n in ((2, 3, 4) if N % 2 == 0 else (2, 3)))      # (2 N alleles tie four ways for an even N only)
        assert any(sorted(c)[1:] == [sorted(c)[1]] * 3 and 0 < sorted(c)[0] < sorted(c)[1] for c in counts)            # such as [1, 2, 2, 2]
        lo, hi = gt & 0xF, gt >> 4
        assert ((lo < hi).any(axis=1) & (lo > hi).any(axis=1)).any()                                                    # hets in both nibble orders
    for d in range(6):
        for layout in (im.LAYOUT_PLANES, im.LAYOUT_SAMPLE_MAJOR):
            want = model(gt, d, layout)
            assert want["bad_site"] == im.NO_SITE
            for subset in SUBSETS:
                got, bad = run_fill(gt, d, layout, subset)
                check_against_model(got, bad, want, subset, (N, S, d, layout, subset))


@pytest.mark.parametrize("S", [1, 67])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 130])
def test_bad_nibbles_give_the_smallest_bad_site(N, S):
    gt, _ = make_gt(S, N, seed=7 * N + S)
    gt = gt.copy()
    # 0xF and 4 .. 14 in either nibble of the first and of the last sample of several sites
    where = [(0, 0, 0xF0)] if S == 1 else [(41, 0, 0x0F), (9, N - 1, 0x40), (9, 0, 0x05), (30, N - 1, 0xE1), (66, 0, 0x2A), (12, N - 1, 0xF3)]
    for i, s, byte in where:
        gt[i, s] = byte
    first = min(i for i, s, b in where)
    for d, layout in itertools.product((0, 1, 4), (im.LAYOUT_PLANES, im.LAYOUT_SAMPLE_MAJOR)):
        want = model(gt, d, layout)
        assert want["bad_site"] == first and len(im.bad_sites(gt)) == len({i for i, s, b in where})
        got, bad = run_fill(gt, d, layout, OUTS)
        check_against_model(got, bad, want, OUTS, (N, S, d, layout))
    # a later bad site alone, and the last sample only
    gt2, _ = make_gt(S, N, seed=3)
    gt2[S - 1, N - 1] = 0x07
    got, bad = run_fill(gt2, 1, im.LAYOUT_SAMPLE_MAJOR, ("pl",))
    assert bad == S - 1


# ---- the context switch ------------------------------------------------------------------------------------------------------------
FIELDS = ["site_status", "n_alleles", "n_alleles_obs", "alleles2acgt", "gl", "pl", "gp", "pl_u8"]


def ctx_args(d=1, layout=im.LAYOUT_SAMPLE_MAJOR, **kw):
    base = dict(seed=5, depth=2, error_rate=0.01, add_fmt_dp=0, add_gl=1, add_gp=1, add_pl=1, do_unobserved=d, out_layout=layout)
    base.update(kw)
    return VcfglArgs(**base)


def tile_arrays(tile):
    return {f: np.ascontiguousarray(tile.numpy(f)) for f in FIELDS}


def assert_tile_is_model(tile, want, ctx=()):
    S = len(want["n_alleles"])
    for k in ("site_status", "n_alleles", "n_alleles_obs", "alleles2acgt"):
        assert np.array_equal(tile.numpy(k).reshape(S, -1), want[k].reshape(S, -1)), (k,) + tuple(ctx)
    for k in OUTS:
        g = np.ascontiguousarray(tile.numpy(k)).reshape(S, -1)
        g = g.view(np.uint32) if k in ("gl", "gp") else g
        assert np.array_equal(g[want["written"]], want[k][want["written"]]), (k,) + tuple(ctx)


@pytest.mark.parametrize("layout", [im.LAYOUT_PLANES, im.LAYOUT_SAMPLE_MAJOR])
@pytest.mark.parametrize("d", [0, 1, 3, 5])
def test_context_tiles_equal_the_stateless_call(d, layout):
    N, S, site0 = 65, 67, 11
    gt, _ = make_gt(S, N, seed=40 + d)
    want = model(gt, d, layout)
    stateless, bad = run_fill(gt, d, layout, OUTS)
    check_against_model(stateless, bad, want, OUTS)
    sim = Simulator(ctx_args(d, layout), N, device=0, max_sites_per_tile=S)
    sim.true_values(1)
    host = sim.simulate(site0, gt, fields=FIELDS)                                       # vgl_simulate_tile (= _async + vgl_tile_wait)
    assert_tile_is_model(host, want, ("host", d, layout))
    dev = sim.new_tile(S, fields=FIELDS, device=DEV)
    for a in dev.arrays.values():
        a.view(torch.uint8).fill_(SENT)
    sim.simulate_device(site0, torch.from_numpy(gt).to(DEV), dev)                       # vgl_simulate_tile_device
    sim.check()
    assert_tile_is_model(dev, want, ("device", d, layout))
    for k in OUTS:                                                                      # and equal to the stateless call, untouched elements included
        assert np.array_equal(as_bytes(dev.arrays[k]).reshape(-1), np.ascontiguousarray(stateless[k]).view(np.uint8).reshape(-1)), k
    # a device tile whose caller does not ask for n_alleles_obs
    few = sim.new_tile(S, fields=["pl"], device=DEV)
    few.struct.n_alleles_obs = None
    sim.simulate_device(site0, torch.from_numpy(gt).to(DEV), few)
    sim.check()
    assert np.array_equal(few.numpy("n_alleles"), want["n_alleles"])
    sim.close()


def test_a_tile_split_at_any_boundary_gives_the_same_arrays():
    N, S = 3, 13
    gt, _ = make_gt(S, N, seed=77)
    sim = Simulator(ctx_args(4), N, device=0, max_sites_per_tile=S)
    sim.true_values(1)
    whole = tile_arrays(sim.simulate(100, gt, fields=FIELDS))
    for k in range(S + 1):
        a, b = tile_arrays(sim.simulate(100, gt[:k], fields=FIELDS)), tile_arrays(sim.simulate(100 + k, gt[k:], fields=FIELDS))
        for f in FIELDS:
            assert np.array_equal(np.concatenate([a[f], b[f]]), whole[f]), (k, f)
    sim.close()


def test_what_true_values_do_not_define_is_refused():
    N, S = 4, 5
    gt, _ = make_gt(S, N, seed=9)
    for kw in (dict(add_fmt_dp=1), dict(add_info_dp=1), dict(add_fmt_ad=1), dict(add_info_ad=1), dict(add_fmt_adf=1), dict(add_info_adf=1),
               dict(add_fmt_adr=1), dict(add_info_adr=1), dict(add_qs=1), dict(add_i16=1)):
        sim = Simulator(ctx_args(**kw), N, device=0, max_sites_per_tile=S)
        with pytest.raises(VglError) as e:
            sim.true_values(1)
        assert e.value.code == _abi.VGL_E_ARG and "vgl_ctx_true_values" in str(e.value), kw
        sim.close()
    sim = Simulator(ctx_args(), N, device=0, max_sites_per_tile=S)
    # a tally, a fetch-GL genotype or a table set first
    for on, off in ((lambda: sim.discordance(1), lambda: sim.discordance(0)), (lambda: sim.fetch_gl("AC"), lambda: sim.fetch_gl(None)),
                    (lambda: sim.set_alleles([(0, 1)] * S), lambda: sim.set_alleles(None))):
        on()
        with pytest.raises(VglError) as e:
            sim.true_values(1)
        assert e.value.code == _abi.VGL_E_ARG
        off()
    sim.true_values(1)
    # ... or afterwards: the tile call refuses
    for on, off in ((lambda: sim.discordance(1), lambda: sim.discordance(0)), (lambda: sim.fetch_gl("AC"), lambda: sim.fetch_gl(None)),
                    (lambda: sim.set_alleles([(0, 1)] * S), lambda: sim.set_alleles(None))):
        on()
        with pytest.raises(VglError) as e:
            sim.simulate(0, gt, fields=FIELDS)
        assert e.value.code == _abi.VGL_E_ARG
        dev = sim.new_tile(S, fields=FIELDS, device=DEV)
        with pytest.raises(VglError) as e:
            sim.simulate_device(0, torch.from_numpy(gt).to(DEV), dev)
        assert e.value.code == _abi.VGL_E_ARG
        off()
    # outputs that need reads
    for f in ("info_dp", "info_ad", "info_adf", "info_adr", "fmt_dp", "fmt_ad", "fmt_adf", "fmt_adr"):
        with pytest.raises(VglError) as e:
            sim.simulate(0, gt, fields=FIELDS + [f])
        assert e.value.code == _abi.VGL_E_ARG and "not defined" in str(e.value), f
        dev = sim.new_tile(S, fields=FIELDS + [f], device=DEV)
        with pytest.raises(VglError) as e:
            sim.simulate_device(0, torch.from_numpy(gt).to(DEV), dev)
        assert e.value.code == _abi.VGL_E_ARG, f
    for kw in (dict(read_capacity=8), dict(read_capacity=8, deviates=True), dict(deviates=True)):
        with pytest.raises(VglError) as e:
            sim.simulate(0, gt, fields=FIELDS, **kw)
        assert e.value.code == _abi.VGL_E_ARG, kw
    # a pileup tile pending, and the gVCF entry point
    ptext, poff = np.zeros(1 << 16, np.uint8), np.zeros(S + 1, np.int64)
    pt = _abi.PileupTile(ptext.ctypes.data, ptext.size, poff.ctypes.data, 0)
    sim._check(sim.lib.vgl_ctx_pileup_next(sim.ctx, C.byref(pt)))
    with pytest.raises(VglError) as e:
        sim.simulate(0, gt, fields=FIELDS)
    assert e.value.code == _abi.VGL_E_ARG and "pileup" in str(e.value)
    items, gtext, roff, boff = np.zeros(S * 16, np.int32), np.zeros(1 << 16, np.uint8), np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int64)
    g = _abi.GvcfTile()
    g.items, g.text, g.text_cap, g.record_offsets, g.block_offsets = items.ctypes.data, gtext.ctypes.data, gtext.size, roff.ctypes.data, boff.ctypes.data
    contig, pos0, dps, t = np.zeros(S, np.int32), np.arange(S, dtype=np.int64), np.array([1], np.int32), C.c_int32()
    tile = sim.new_tile(S, fields=FIELDS)
    assert sim.lib.vgl_simulate_tile_gvcf_async(sim.ctx, 0, S, gt.ctypes.data, contig.ctypes.data, pos0.ctypes.data, dps.ctypes.data, 1, tile.byref(), C.byref(g),
                                                C.byref(t)) == _abi.VGL_E_ARG
    # the context still works
    assert_tile_is_model(sim.simulate(0, gt, fields=FIELDS), model(gt, 1, im.LAYOUT_SAMPLE_MAJOR))
    sim.close()


def test_a_bad_site_is_reported_with_its_absolute_index():
    N, S, site0 = 65, 20, 1000
    gt, _ = make_gt(S, N, seed=13)
    bad = gt.copy()
    bad[7, N - 1] = 0xF2
    bad[15, 0] = 0x4F
    sim = Simulator(ctx_args(), N, device=0, max_sites_per_tile=S)
    sim.true_values(1)
    with pytest.raises(VglError) as e:
        sim.simulate(site0, bad, fields=FIELDS)
    assert e.value.code == _abi.VGL_E_ARG and "site %d:" % (site0 + 7) in str(e.value)
    want = model(gt, 1, im.LAYOUT_SAMPLE_MAJOR)
    assert_tile_is_model(sim.simulate(site0, gt, fields=FIELDS), want)                  # the word is clean again
    dev = sim.new_tile(S, fields=FIELDS, device=DEV)
    sim.simulate_device(site0 + S, torch.from_numpy(bad[10:]).to(DEV), sim.new_tile(S - 10, fields=FIELDS, device=DEV))
    sim.simulate_device(site0, torch.from_numpy(bad).to(DEV), dev)
    with pytest.raises(VglError) as e:
        sim.check()
    assert e.value.code == _abi.VGL_E_ARG and "site %d:" % (site0 + 7) in str(e.value)  # the smallest of the tiles since the last check
    sim.simulate_device(site0, torch.from_numpy(gt).to(DEV), dev)
    sim.check()
    assert_tile_is_model(dev, want)
    sim.close()


def test_simulated_tiles_around_a_true_value_tile_are_bit_identical():
    N, S = 65, 33
    gt, _ = make_gt(S, N, seed=21)
    fields = ["site_status", "n_alleles", "n_alleles_obs", "alleles2acgt", "gl", "pl", "gp"]
    sim = Simulator(ctx_args(depth=3, error_rate=0.05), N, device=0, max_sites_per_tile=S)
    first = sim.simulate(5, gt, fields=fields)
    before = {f: first.numpy(f).copy() for f in fields}
    assert len(np.unique(before["pl"])) > 3                                           # (a simulated tile, not a true-value one)
    sim.true_values(1)
    assert_tile_is_model(sim.simulate(5, gt, fields=FIELDS), model(gt, 1, im.LAYOUT_SAMPLE_MAJOR))
    sim.true_values(0)
    after = sim.simulate(5, gt, fields=fields)
    for f in fields:
        assert np.array_equal(after.numpy(f).view(np.uint8), before[f].view(np.uint8)), f
    sim.close()
