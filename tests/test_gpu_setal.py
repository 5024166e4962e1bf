"""The device relabelling (csrc/vgl_setal.hip: vgl_setal_apply_device) against the numpy model of misc/setAlleles
(tests/setal_model.py), bit for bit: synthetic tiles of 37 sites over sample counts around a wavefront, a 256-lane workgroup and its
LDS chunk, both layouts, every old and new allele count, skipped sites, samples without reads, -inf entries, int32 and one-byte PL
together and alone, and the refusal of a target with an allele the record does not have."""
import numpy as np
import pytest
import torch

import setal_model as sm
from vcfgl_amd import _abi, setalleles

pytestmark = pytest.mark.gpu
PLANES, SAMPLE_MAJOR = _abi.VGL_LAYOUT_PLANES, _abi.VGL_LAYOUT_SAMPLE_MAJOR
S, G, A = 37, 15, 5
GUARD = 64
# (old count, new count) of site i: every pair with new <= old, 2 .. 5
COUNTS = [(o, n) for o in range(2, 6) for n in range(2, o + 1)]


def make_tile(N, layout, seed):
    """a tile as the simulator leaves it, and the targets: dict of numpy arrays"""
    rng = np.random.default_rng(seed)
    st = np.zeros(S, np.int32)
    st[[3, 17]] = [-3, -4]                                        # skipped sites: nothing of theirs may change
    st[5] = 1
    nA = np.array([COUNTS[i % len(COUNTS)][0] for i in range(S)], np.int32)
    a2b = np.full((S, 5), -1, np.int8)
    targets = []
    for i in range(S):
        a2b[i, :nA[i]] = rng.permutation(5)[:nA[i]]
        targets.append(tuple(int(c) for c in rng.permutation(a2b[i, :nA[i]])[:COUNTS[i % len(COUNTS)][1]]))
    dp = rng.integers(0, 6, (S, N)).astype(np.int32)
    dp[:, rng.random(N) < 0.2] = 0                                # samples without reads
    dp[1, 0] = 3                                                  # (the all -inf sample below has reads)
    qs = rng.random((S, A)).astype(np.float32)
    t = {"st": st, "nA": nA, "a2b": a2b, "targets": targets, "dp": dp, "qs": qs, "N": N, "layout": layout}
    fills = {"gl": sm.FLOAT_MISSING, "pl": np.int32(-2 ** 31), "gp": sm.FLOAT_MISSING, "pl_u8": np.uint8(255)}
    dt = {"gl": np.uint32, "pl": np.int32, "gp": np.uint32, "pl_u8": np.uint8}
    for k in sm.KINDS:
        t[k] = np.full(S * G * N + GUARD, fills[k] if layout == PLANES else 0, dt[k])
        t[k][S * G * N:] = 0x5A
    for i in range(S):
        nG = sm.n_gt(int(nA[i]))
        miss = dp[i] == 0
        gl = (-rng.random((nG, N)) * 40).astype(np.float32)
        gl[rng.integers(0, nG, N), np.arange(N)] = 0.0
        gl[rng.random((nG, N)) < 0.1] = -np.inf
        pl = rng.integers(0, 256, (nG, N)).astype(np.int32)
        pl[rng.integers(0, nG, N), np.arange(N)] = 0
        gp = rng.random((nG, N)).astype(np.float32)
        gp[rng.random((nG, N)) < 0.1] = 0.0
        if i == 1:                                                # a sample whose kept genotypes are all -inf: only dropped ones are finite
            o2n = sm.allele_map([int(c) for c in a2b[i, :nA[i]]], list(targets[i]))
            g2g = sm.genotype_map(o2n)
            gl[:, 0] = [-np.inf if h >= 0 else 0.0 for h in g2g]
        glb, gpb = gl.view(np.uint32).copy(), gp.view(np.uint32).copy()
        glb[:, miss] = sm.FLOAT_MISSING
        gpb[:, miss] = sm.FLOAT_MISSING
        u8 = pl.astype(np.uint8)
        u8[:, miss] = 255
        pl[:, miss] = -2 ** 31
        for k, v in (("gl", glb), ("pl", pl), ("gp", gpb), ("pl_u8", u8)):
            sm.site_store(t[k][:S * G * N], i, G, N, v, layout, fills[k])
    return t


@pytest.fixture(scope="module")
def tiles():
    """the synthetic tiles and the model's relabelling of each: computed once, shared, never changed"""
    out = {}
    for layout in (PLANES, SAMPLE_MAJOR):
        for N in (1, 63, 64, 65, 257):
            t = make_tile(N, layout, 1000 * layout + N)
            n = S * G * N
            want, bad = sm.relabel_tile(t["targets"], t["st"], t["nA"], t["a2b"], N, G, A, layout, qs=t["qs"], fmt_dp=t["dp"],
                                        gl=t["gl"][:n], pl=t["pl"][:n], gp=t["gp"][:n], pl_u8=t["pl_u8"][:n])
            assert bad == sm.NO_SITE
            out[layout, N] = (t, want)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(t, kinds, targets=None, with_qs=True):
    N, layout = t["N"], t["layout"]
    d = {k: dev(t[k]) for k in kinds}
    st, nA, a2b, dp = dev(t["st"]), dev(t["nA"]), dev(t["a2b"]), dev(t["dp"])
    qs = dev(t["qs"]) if with_qs else None
    table = dev(setalleles.build_table(t["targets"] if targets is None else targets))
    view = {"gl": torch.float32, "gp": torch.float32}
    args = {k: (d[k].view(view[k]) if k in view else d[k]) for k in kinds}
    bad, _ = setalleles.apply_into(table, st, nA, a2b, N, qs=qs, fmt_dp=dp, max_genotypes=G, max_alleles=A, layout=layout, **args)
    torch.cuda.synchronize()
    got = {k: d[k].cpu().numpy() for k in kinds}
    got.update(n_alleles=nA.cpu().numpy(), a2b=a2b.cpu().numpy(), st=st.cpu().numpy(), dp=dp.cpu().numpy())
    if with_qs:
        got["qs"] = qs.cpu().numpy()
    return got, int(bad.item())


def compare(t, want, got, kinds, sites=None):
    N, layout = t["N"], t["layout"]
    n = S * G * N
    keep = np.ones(S, bool) if sites is None else sites
    assert np.array_equal(got["n_alleles"][keep], want["n_alleles"][keep]) and np.array_equal(got["a2b"][keep], want["a2b"][keep])
    assert np.array_equal(got["st"], t["st"]) and np.array_equal(got["dp"], t["dp"])
    mask = sm.defined_mask(t["st"], want["n_alleles"], N, G, layout) & np.repeat(keep, G * N)
    for k in kinds:
        g, w = got[k][:n], want[k]
        if k == "pl":
            g, w = g.view(np.uint32), w.view(np.uint32)
        ok = g == w
        if k in ("gl", "gp"):                                     # a NaN that arithmetic made (-inf - -inf, 0 / 0): its sign is the machine's
            ok |= sm.is_nan_bits(g) & sm.is_nan_bits(w) & (g != sm.FLOAT_MISSING) & (w != sm.FLOAT_MISSING)
        badi = np.flatnonzero(mask & ~ok)
        assert badi.size == 0, (k, N, layout, badi[:8], g[badi[:8]], w[badi[:8]])
        assert bool((got[k][n:] == t[k][n:]).all()), (k, "guard")


@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_all_arrays_against_the_model(tiles, layout, N):
    t, want = tiles[layout, N]
    got, bad = run(t, sm.KINDS)
    assert bad == sm.NO_SITE
    compare(t, want, got, sm.KINDS)
    assert np.array_equal(got["qs"], want["qs"])
    # skipped sites: every byte as it was (both layouts, whole slab)
    for i in np.flatnonzero(t["st"] < 0):
        for k in sm.KINDS:
            assert np.array_equal(got[k][i * G * N:(i + 1) * G * N], t[k][i * G * N:(i + 1) * G * N])
    # the sample whose kept genotypes are all -inf: -inf - -inf is NaN (its bits are not compared)
    n1 = sm.n_gt(int(want["n_alleles"][1]))
    v = sm.site_view(got["gl"][:S * G * N], 1, G, N, n1, layout)[:, 0]
    assert bool(sm.is_nan_bits(v).all()) and not bool((v == sm.FLOAT_MISSING).any())


@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
@pytest.mark.parametrize("kinds", [("pl",), ("pl_u8",), ("gl",), ("gp", "pl_u8")])
def test_arrays_alone(tiles, layout, kinds):
    t, want = tiles[layout, 65]
    got, bad = run(t, kinds, with_qs=False)
    assert bad == sm.NO_SITE
    compare(t, want, got, kinds)


@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
def test_absent_target_allele_is_refused(tiles, layout):
    t, want = tiles[layout, 65]
    targets = list(t["targets"])
    refused = []
    for i in (24, 11, 3):                                         # 3 is a skipped site: not looked at
        absent = [c for c in range(5) if c not in t["a2b"][i, :t["nA"][i]]]
        if absent and t["st"][i] >= 0:
            refused.append(i)
        targets[i] = (int(t["a2b"][i, 0]), absent[0]) if absent else targets[i]
    assert refused == [24, 11]
    got, bad = run(t, sm.KINDS, targets=targets)
    assert bad == 11
    keep = np.ones(S, bool)
    keep[refused] = False
    compare(t, want, got, sm.KINDS, sites=keep)                   # every other site as without the refusal


def test_bad_arguments_are_refused_before_any_launch():
    lib = _abi.load_library()
    x = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = x.data_ptr()
    ok = [0, 1, 1, 10, 4, PLANES, p, p, p, p, None, None, None, None, None, None, p, p, 1 << 20, None]
    for k, v in [(1, 0), (3, 16), (3, 0), (4, 6), (5, 2), (6, None), (16, None), (17, None), (18, 8)]:
        a = list(ok)
        a[k] = v
        assert lib.vgl_setal_apply_device(*a) == _abi.VGL_E_ARG, (k, v)
    a = list(ok)
    a[15] = p                                                     # pl_u8 without fmt_dp
    assert lib.vgl_setal_apply_device(*a) == _abi.VGL_E_ARG
