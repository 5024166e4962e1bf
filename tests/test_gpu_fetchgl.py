"""The device fetch-GL formatter (csrc/vgl_fetchgl.hip: vgl_fetchgl_format_device) against the Python model of misc/fetchGl
(tests/fetchgl_model.py): synthetic tiles over sample counts around a wavefront, a 256-lane workgroup and its chunk loop, both GL
layouts, 10 and 15 genotype planes, allele tables of 1 .. 5 alleles, every site status, all 25 allele pairs, both value modes on the
whole value set, and the capacity contract."""
import numpy as np
import pytest
import torch

import fetchgl_model as fm
from vcfgl_amd import _abi, fetchgl

pytestmark = pytest.mark.gpu
STATUSES = [0, 1, -3, -4]                # kept, no reads (kept), invariant (skipped), empty (skipped)
PLANES, SAMPLE_MAJOR = _abi.VGL_LAYOUT_PLANES, _abi.VGL_LAYOUT_SAMPLE_MAJOR


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def values():
    """the value set and the model's text of every value in both modes: computed once, shared, never changed"""
    pats = fm.value_set()
    table = [{int(b): fm.fmt_value_bits(b, mode) for b in pats} for mode in (fm.FLOAT, fm.TEXT)]
    return pats, table


def site_tables(S, seed, G):
    """n_alleles 1 .. 5, every status, allele tables that are random arrangements of A, C, G, T, <*>: any pair is present at some
    sites and absent at others.  With more than two sites the first and the last have no line (skipped / one allele only)."""
    rng = np.random.default_rng(seed)
    st = np.array([STATUSES[(i + seed) % 4] if rng.random() < 0.4 else 0 for i in range(S)], np.int32)
    nA = rng.integers(1, 6, S).astype(np.int32)
    a2b = np.stack([rng.permutation(5) for _ in range(S)]).astype(np.int8)
    if S > 2:
        st[0] = -4
        st[-1] = 0
        nA[-1] = 0
    return st, nA, a2b


def run(st, nA, a2b, gl_bits, layout, G, a, b, mode, cap=None, guard=0):
    S = len(st)
    want_total = None
    off = torch.full((S + 1,), -7, dtype=torch.int64, device="cuda")
    if cap is None:                                              # first the size, with no room at all
        fetchgl.format_into(dev(st), dev(nA), dev(a2b), dev(gl_bits).view(torch.float32), a, b, mode, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                            off, max_genotypes=G, layout=layout)
        want_total = cap = int(off[-1])
    buf = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    fetchgl.format_into(dev(st), dev(nA), dev(a2b), dev(gl_bits).view(torch.float32), a, b, mode, buf[:cap], off, max_genotypes=G, layout=layout)
    torch.cuda.synchronize()
    assert want_total is None or int(off[-1]) == want_total
    return buf.cpu().numpy(), off.cpu().numpy()


def check(st, nA, a2b, gl_bits, layout, G, a, b, mode, table=None):
    want, woff = fm.render(st, nA, a2b, gl_bits, layout, G, a, b, mode) if table is None else render_cached(st, nA, a2b, gl_bits, layout, G, a, b, table[mode])
    buf, off = run(st, nA, a2b, gl_bits, layout, G, a, b, mode, guard=64)
    assert np.array_equal(off, woff), (off[:8], woff[:8])
    got = bytes(buf[:len(want)])
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"first difference at byte {k}: {got[max(0, k - 40):k + 40]!r} vs {want[max(0, k - 40):k + 40]!r}")
    assert bool((buf[len(want):] == 0xA5).all())                 # exact capacity: the guard bytes behind the text are untouched
    return want, woff


def render_cached(st, nA, a2b, gl_bits, layout, G, a, b, text_of):
    """fetchgl_model.render with the module's table of formatted values"""
    S = len(st)
    N = gl_bits.size // (S * G)
    flat = gl_bits.reshape(S, G * N)
    parts, offsets, pos = [], [0], 0
    for i in range(S):
        n = min(max(int(nA[i]), 0), 5)
        nG = n * (n + 1) // 2
        g = fm.genotype_index([fm.LETTERS[c] for c in a2b[i][:n]], fm.LETTERS[a] + fm.LETTERS[b]) if st[i] >= 0 else None
        if g is not None and nG <= G:
            row = flat[i][g * N:(g + 1) * N] if layout == PLANES else flat[i][g:N * nG:nG]
            t = (",".join(text_of[int(x)] for x in row) + "\n").encode()
            parts.append(t)
            pos += len(t)
        offsets.append(pos)
    return b"".join(parts), np.array(offsets, dtype=np.int64)


@pytest.mark.parametrize("G", [10, 15])
@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
@pytest.mark.parametrize("S", [1, 7, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_synthetic_tiles_equal_the_model(values, N, S, layout, G):
    pats, table = values
    seed = N * 7 + S * 3 + layout * 2 + G
    rng = np.random.default_rng(seed)
    st, nA, a2b = site_tables(S, seed, G)
    gl = pats[rng.integers(0, len(pats), S * G * N)]
    a, b, mode = seed % 5, (seed // 5) % 5, seed % 2
    want, woff = check(st, nA, a2b, gl, layout, G, a, b, mode, table)
    if S > 2:
        assert woff[1] == 0 and woff[-1] == woff[-2]             # the first and the last site have no line
    if S == 300:
        assert 0 < want.count(b"\n") < int((st >= 0).sum())      # some kept sites lack the genotype, some have it


@pytest.mark.parametrize("a", range(5))
@pytest.mark.parametrize("b", range(5))
def test_every_allele_pair(values, a, b):
    pats, table = values
    rng = np.random.default_rng(a * 5 + b)
    S, N = 40, 65
    for layout, G in ((PLANES, 15), (SAMPLE_MAJOR, 15), (PLANES, 10)):
        st, nA, a2b = site_tables(S, a * 5 + b + G, G)
        gl = pats[rng.integers(0, len(pats), S * G * N)]
        for mode in (fm.FLOAT, fm.TEXT):
            want, _ = check(st, nA, a2b, gl, layout, G, a, b, mode, table)
            assert want.count(b"\n") > 0


@pytest.mark.parametrize("layout", [PLANES, SAMPLE_MAJOR])
@pytest.mark.parametrize("mode", [fm.FLOAT, fm.TEXT])
def test_the_whole_value_set(values, mode, layout):
    """every value of the set in the requested genotype's row: sites of four alleles A, C, G, T and the pair (C, C) -> g = 2"""
    pats, table = values
    N, G = 1000, 10
    S = (len(pats) + N - 1) // N
    row = np.resize(pats, S * N).reshape(S, N)
    gl = np.random.default_rng(5).integers(0, 2 ** 32, (S, G, N), dtype=np.uint64).astype(np.uint32)
    if layout == PLANES:
        gl[:, 2, :] = row
    else:
        gl.reshape(S, N, G)[:, :, 2] = row                      # nG = 10 = G: sample s's values at s * 10
    st, nA = np.zeros(S, np.int32), np.full(S, 4, np.int32)
    a2b = np.tile(np.array([0, 1, 2, 3, -1], np.int8), (S, 1))
    want, _ = check(st, nA, a2b, gl.reshape(-1), layout, G, 1, 1, mode, table)
    assert want.count(b"\n") == S
    # the plain model (no table) on the first sites: the cached rendering above is the same function
    k = 3
    w2, _ = fm.render(st[:k], nA[:k], a2b[:k], gl[:k].reshape(-1), layout, G, 1, 1, mode)
    assert want.startswith(w2)


def test_capacity_contract_and_bad_arguments(values):
    pats, table = values
    S, N, G = 30, 77, 10
    rng = np.random.default_rng(2)
    st, nA, a2b = site_tables(S, 4, G)
    gl = pats[rng.integers(0, len(pats), S * G * N)]
    want, woff = render_cached(st, nA, a2b, gl, PLANES, G, 0, 1, table[fm.TEXT])
    total = len(want)
    assert total > 0
    buf, off = run(st, nA, a2b, gl, PLANES, G, 0, 1, fm.TEXT, cap=total - 1)
    assert int(off[-1]) == total and bool((buf == 0xA5).all())  # one byte short: the size it needs, nothing written
    assert np.array_equal(off, woff)
    buf, off = run(st, nA, a2b, gl, PLANES, G, 0, 1, fm.TEXT, cap=total + 3, guard=5)
    assert bytes(buf[:total]) == want and bool((buf[total:] == 0xA5).all())
    assert fetchgl.lines(np.arange(1, S + 1), buf[:total], off) == fm.lines(np.arange(1, S + 1), want, woff)
    lib = _abi.load_library()
    d = [dev(x) for x in (st, nA, a2b, gl)]
    o = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(S * N * 4, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")

    def call(n=N, s=S, g=G, layout=PLANES, a=0, b=1, mode=0, ws_bytes=ws.numel()):
        return lib.vgl_fetchgl_format_device(0, n, s, g, layout, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), a, b, mode,
                                             dst.data_ptr(), total, o.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call() == _abi.VGL_OK
    for kw in (dict(a=5), dict(a=-1), dict(b=5), dict(mode=2), dict(mode=-1), dict(layout=2), dict(g=0), dict(g=16), dict(n=0), dict(s=-1),
               dict(ws_bytes=S * N * 4 - 1)):
        assert call(**kw) == _abi.VGL_E_ARG, kw
    assert call(s=0) == _abi.VGL_OK                              # no sites: offsets[0] = 0
    torch.cuda.synchronize()
    assert int(o[0]) == 0
