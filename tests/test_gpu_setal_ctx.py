"""vgl_ctx_set_alleles / Simulator.set_alleles: a tile submitted with a target table equals the numpy model of misc/setAlleles
(tests/setal_model.py) applied to the plain tile of the same seed -- both RNG modes, both layouts, through the array and the text
entry points, after a rerun on the sibling context -- and a target with an allele the record lacks gives VGL_E_SETAL naming the site."""
import ctypes as C

import numpy as np
import pytest

import setal_model as sm
import synth
from vcfgl_amd import Simulator, VcfglArgs, VglError, _abi

pytestmark = pytest.mark.gpu
FIELDS = ["site_status", "n_alleles", "n_alleles_obs", "alleles2acgt", "info_dp", "qs", "fmt_dp", "gl", "pl", "gp", "pl_u8"]
PLANES, SAMPLE_MAJOR = _abi.VGL_LAYOUT_PLANES, _abi.VGL_LAYOUT_SAMPLE_MAJOR


def sim_args(mode=_abi.VGL_RNG_TILE, layout=SAMPLE_MAJOR, **kw):
    base = dict(seed=11, depth=3, error_rate=0.05, add_fmt_dp=1, add_info_dp=1, add_pl=1, add_gp=1, add_qs=1, do_unobserved=4, out_layout=layout)
    base.update(kw)
    a = VcfglArgs(**base)
    a.rng_mode = mode
    a.beta_sampler = _abi.VGL_BETA_STD if mode == _abi.VGL_RNG_SERIAL else _abi.VGL_BETA_RAND48
    return a


def subset_targets(tile, seed):
    """for every site a random arrangement of some of its own alleles: 2, 3, 4, 5, 2, ... of them (as many as it has, at most)"""
    rng = np.random.default_rng(seed)
    nA, a2b = tile.numpy("n_alleles"), tile.numpy("alleles2acgt")
    out = []
    for i in range(len(nA)):
        n = int(nA[i])
        own = [int(c) for c in a2b[i][:n]] if n >= 2 else [0, 1]
        out.append(tuple(int(c) for c in rng.permutation(own)[:min(2 + i % 4, len(own))]))
    return out


def model(plain, targets, N, G, A, layout):
    bits = lambda f: np.ascontiguousarray(plain.numpy(f)).reshape(-1).view(np.uint32)
    return sm.relabel_tile(targets, plain.numpy("site_status"), plain.numpy("n_alleles"), plain.numpy("alleles2acgt"), N, G, A, layout,
                           qs=plain.numpy("qs"), fmt_dp=plain.numpy("fmt_dp"), gl=bits("gl"), pl=np.ascontiguousarray(plain.numpy("pl")).reshape(-1),
                           gp=bits("gp"), pl_u8=np.ascontiguousarray(plain.numpy("pl_u8")).reshape(-1))


def assert_tile(got, want, plain, N, G, layout):
    st = plain.numpy("site_status")
    assert (st >= 0).any()
    assert np.array_equal(got.numpy("site_status"), st)
    assert np.array_equal(got.numpy("n_alleles"), want["n_alleles"]) and np.array_equal(got.numpy("alleles2acgt"), want["a2b"])
    assert np.array_equal(got.numpy("qs").view(np.uint32), want["qs"].view(np.uint32))
    for f in ("fmt_dp", "info_dp", "n_alleles_obs"):
        assert np.array_equal(got.numpy(f), plain.numpy(f)), f
    mask = sm.defined_mask(st, want["n_alleles"], N, G, layout)
    for f in sm.KINDS:
        g = np.ascontiguousarray(got.numpy(f)).reshape(-1)
        g = g.view(np.uint32) if g.dtype.itemsize == 4 else g
        w = want[f].view(np.uint32) if want[f].dtype.itemsize == 4 else want[f]
        ok = g == w
        if f in ("gl", "gp"):
            ok |= sm.is_nan_bits(g) & sm.is_nan_bits(w) & (g != sm.FLOAT_MISSING) & (w != sm.FLOAT_MISSING)
        bad = np.flatnonzero(mask & ~ok)
        assert bad.size == 0, (f, bad[:8], g[bad[:8]], w[bad[:8]])


@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
@pytest.mark.parametrize("mode", [_abi.VGL_RNG_TILE, _abi.VGL_RNG_SERIAL], ids=["tile", "serial"])
def test_set_alleles_equals_the_model_on_the_plain_tile(mode, layout):
    N, S, site0 = 65, 64, 0 if mode == _abi.VGL_RNG_SERIAL else 7
    args = sim_args(mode, layout)
    gt = synth.acgt_sites(S, N, seed=21, missing=0.03)
    ref = Simulator(args, N, device=0, max_sites_per_tile=S)
    plain = ref.simulate(site0, gt, fields=FIELDS)
    G, A = ref.G, ref.A
    ref.close()
    targets = subset_targets(plain, 5)
    assert {len(t) for t in targets} >= {2, 3, 4}
    want, bad = model(plain, targets, N, G, A, layout)
    assert bad == sm.NO_SITE
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    sim.set_alleles(targets, first_site=site0)
    got = sim.simulate(site0, gt, fields=FIELDS)
    assert_tile(got, want, plain, N, G, layout)
    if mode == _abi.VGL_RNG_TILE:
        # a tile outside the table is refused at submit; switched off, the tile is the plain one again
        with pytest.raises(VglError) as e:
            sim.simulate(site0 + 1, gt, fields=FIELDS)
        assert e.value.code == _abi.VGL_E_ARG
        sim.set_alleles(None)
        again = sim.simulate(site0, gt, fields=FIELDS)
        for f in FIELDS:
            assert np.array_equal(np.ascontiguousarray(again.numpy(f)).view(np.uint8), np.ascontiguousarray(plain.numpy(f)).view(np.uint8)), f
    sim.close()


def test_the_text_entry_point_formats_the_relabelled_arrays():
    """vgl_simulate_tile_text_async with a table: the arrays it hands back are the model's, and the text differs from the plain tile's"""
    N, S = 65, 64
    args = sim_args()
    gt = synth.acgt_sites(S, N, seed=22, missing=0.03)
    texts = []
    for with_table in (False, True):
        sim = Simulator(args, N, device=0, max_sites_per_tile=S)
        if with_table:
            sim.set_alleles(targets)
        cap = int(sim.lib.vgl_ctx_text_bound(sim.ctx, S))
        text, off, t = np.zeros(cap, np.uint8), np.zeros(S + 1, np.int64), C.c_int32()
        tile = sim.new_tile(S, fields=FIELDS)
        sim._check(sim.lib.vgl_simulate_tile_text_async(sim.ctx, 0, S, gt.ctypes.data, tile.byref(), text.ctypes.data, cap, off.ctypes.data, C.byref(t)))
        sim._check(sim.lib.vgl_tile_wait(sim.ctx, t.value))
        texts.append(bytes(text[:off[S]]))
        if not with_table:
            plain, targets = tile, subset_targets(tile, 6)
        else:
            want, bad = model(plain, targets, N, sim.G, sim.A, args.out_layout)
            assert bad == sm.NO_SITE
            assert_tile(tile, want, plain, N, sim.G, args.out_layout)
        sim.close()
    assert texts[0] != texts[1] and 0 < len(texts[1]) < len(texts[0])


@pytest.mark.parametrize("entry", ["arrays", "text"])
def test_a_tile_that_is_run_again_is_relabelled_from_the_rerun(monkeypatch, entry):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (the hooks build): every tile draws deeper than the staging capacity and is run again on the
    sibling context, in sub-tiles; the relabelled tile is that of the rerun's values"""
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    N, S, site0 = 40, 2100, 3
    args = sim_args(depth=20, seed=42, error_rate=0.01)
    gt = synth.acgt_sites(S, N, seed=S, missing=0.03)
    sim = Simulator(args, N, max_sites_per_tile=S, hooks=True)
    assert sim.info()["read_cap"] == 8
    plain = sim.simulate(site0, gt, fields=FIELDS)
    assert int(plain.numpy("fmt_dp").max()) > 8
    targets = subset_targets(plain, 7)
    want, bad = model(plain, targets, N, sim.G, sim.A, args.out_layout)
    sim.set_alleles(targets, first_site=site0)
    if entry == "arrays":
        got = sim.simulate(site0, gt, fields=FIELDS)
    else:
        cap = int(sim.lib.vgl_ctx_text_bound(sim.ctx, S))
        text, off, t = np.zeros(cap, np.uint8), np.zeros(S + 1, np.int64), C.c_int32()
        got = sim.new_tile(S, fields=FIELDS)
        sim._check(sim.lib.vgl_simulate_tile_text_async(sim.ctx, site0, S, gt.ctypes.data, got.byref(), text.ctypes.data, cap, off.ctypes.data, C.byref(t)))
        sim._check(sim.lib.vgl_tile_wait(sim.ctx, t.value))
        assert off[S] > 0
    assert_tile(got, want, plain, N, sim.G, args.out_layout)
    sim.close()


def test_an_absent_target_allele_is_refused_with_the_site():
    N, S, site0 = 65, 64, 100
    args = sim_args(do_unobserved=1, error_rate=0.001)              # two true alleles per site and few errors: most records lack a base
    gt = synth.acgt_sites(S, N, seed=23, missing=0.03, n_alleles=2)
    sim = Simulator(args, N, device=0, max_sites_per_tile=S)
    plain = sim.simulate(site0, gt, fields=FIELDS)
    nA, a2b, st = plain.numpy("n_alleles"), plain.numpy("alleles2acgt"), plain.numpy("site_status")
    lacking = [i for i in range(S) if st[i] >= 0 and not {0, 1, 2, 3} <= {int(c) for c in a2b[i][:nA[i]]}]
    assert lacking, "every record of the tile has A, C, G and T: the case is not exercised"
    sim.set_alleles([(0, 1, 2, 3)] * S, first_site=site0)
    with pytest.raises(VglError) as e:
        sim.simulate(site0, gt, fields=FIELDS)
    assert e.value.code == _abi.VGL_E_SETAL and ("site %d:" % (site0 + lacking[0])) in str(e.value)
    # the context's own refusals
    sim.set_alleles(None)
    t8 = np.zeros((1, 8), np.int8)
    for entry in ([1, 0, -1, -1, -1, -1, 0, 0], [6, 0, 1, 2, 3, 4, 0, 0], [2, 0, 5, -1, -1, -1, 0, 0], [3, 0, 1, 0, -1, -1, 0, 0]):
        t8[0] = entry
        assert sim.lib.vgl_ctx_set_alleles(sim.ctx, t8.ctypes.data, 0, 1) == _abi.VGL_E_ARG, entry
    sim.close()
    for kw in (dict(add_fmt_ad=1), dict(add_info_ad=1), dict(add_fmt_adf=1), dict(add_info_adr=1), dict(do_gvcf=1)):
        s2 = Simulator(sim_args(**kw), N, device=0, max_sites_per_tile=S)
        with pytest.raises(VglError) as e:
            s2.set_alleles([(0, 1)] * S)
        assert e.value.code == _abi.VGL_E_ARG
        s2.close()
