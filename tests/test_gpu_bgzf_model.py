"""The device BGZF compressor (vgl_bgzf.hip) equals its reference model (tests/bgzf_model.py) byte for byte, member by member:
the model corpus, every length from 1 to 300 and the lengths next to multiples of 64 (CRC slices), 512 (parse segments) and
0xff00 (members), unaligned sources, an input of more than 512 members (the member kernel's grid-stride loop), and the host batch
API (vgl_bgzf_host_*) at its edges."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_model as bm

pytestmark = pytest.mark.gpu
M = bm.MEMBER


def _dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to("cuda")


def _compress(t):
    from vcfgl_amd import bgzf
    return bgzf.compress(t).cpu().numpy().tobytes()


def _equal_to_model(raw, data, only=None):
    got = bm.split_members(raw)
    assert len(got) == -(-len(data) // M)
    for k, g in enumerate(got):
        if only is not None and k not in only:
            continue
        m = bm.member(data[k * M:(k + 1) * M])
        assert g == m.raw, (k, len(g), len(m.raw), m.mode)


@pytest.mark.parametrize("name", sorted(bm.corpus()))
def test_corpus_equals_model(name):
    data = bm.corpus()[name]
    raw = _compress(_dev(data))
    _equal_to_model(raw, data)
    for g in bm.split_members(raw):
        bm.inflate_member(g)


def test_lengths_1_to_300_and_boundaries_equal_model():
    rng = np.random.default_rng(11)
    words = [b"0/0", b"0/1", b"1/1", b"-0.30103", b"\t", b"\n", b"PASS", b"chr1"]
    text = b"".join(words[i] for i in rng.integers(0, len(words), 40000))
    lengths = list(range(1, 301)) + sorted({k * q + e for q in (64, 512) for k in (2, 5, 17, 127) for e in (-1, 0, 1)}) + [M - 1, M, M + 1]
    for n in lengths:
        data = text[:n] if n % 2 else bytes(rng.integers(0, 256, n, dtype=np.uint8)) if n % 3 == 0 else text[len(text) - n:]
        _equal_to_model(_compress(_dev(data)), data)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_source_equals_aligned(shift):
    data = bm.corpus()["words"][:M + 3000]
    aligned = _dev(data)
    unal = _dev(bytes(shift) + data)[shift:]             # the same bytes at an address that is not 4-byte aligned
    assert aligned.data_ptr() % 4 == 0 and unal.data_ptr() % 4 == shift
    a, u = _compress(aligned), _compress(unal)
    assert a == u
    _equal_to_model(u, data)


def test_more_than_512_members():
    n_members = 600
    rng = np.random.default_rng(12)
    words = [b"0/0", b"0/1", b"1/1", b"-0.30103", b"-1.2", b"\t", b"\n", b"PASS", b"chr1", b"GT:DP"]
    data = b"".join(words[i] for i in rng.integers(0, len(words), 14_000_000))[:n_members * M - 12345]
    assert len(data) < 40 << 20
    raw = _compress(_dev(data))
    got = bm.split_members(raw)
    assert len(got) == n_members
    for k, g in enumerate(got):
        piece = data[k * M:(k + 1) * M]
        assert zlib.decompress(g[18:-8], -15) == piece and int.from_bytes(g[-8:-4], "little") == zlib.crc32(piece), k
    _equal_to_model(raw, data, only={0, 511, 512, 513, n_members - 1})


def test_host_batch_api_edges():
    from vcfgl_amd import _abi
    lib = _abi.load_library()
    cap = 3 * M + 100
    h = C.c_void_p()
    assert lib.vgl_bgzf_host_create(0, cap, C.byref(h)) == _abi.VGL_OK and h.value
    try:
        rng = np.random.default_rng(13)
        words = [b"0/1", b"1/1", b"\t", b"PASS", b"-0.5"]
        text = b"".join(words[i] for i in rng.integers(0, len(words), 100000))
        inputs = [text[:cap], text[7:7 + 2 * M + 1], b""]
        bufs = [C.create_string_buffer(x, max(1, len(x))) for x in inputs]
        t = [C.c_int32(-1) for _ in inputs]
        out, out_n = C.c_void_p(), C.c_int64()

        def wait(ticket):
            rc = lib.vgl_bgzf_host_wait(h, ticket, C.byref(out), C.byref(out_n))
            return rc, (C.string_at(out.value, out_n.value) if rc == _abi.VGL_OK and out_n.value else b"")

        # two batches in flight (n = max_batch), a third submit refused
        assert lib.vgl_bgzf_host_submit(h, bufs[0], len(inputs[0]), C.byref(t[0])) == _abi.VGL_OK
        assert lib.vgl_bgzf_host_submit(h, bufs[1], len(inputs[1]), C.byref(t[1])) == _abi.VGL_OK
        assert t[0].value != t[1].value
        x = C.c_int32(-1)
        assert lib.vgl_bgzf_host_submit(h, bufs[2], 0, C.byref(x)) == _abi.VGL_E_ARG and b"in flight" in lib.vgl_last_error()
        assert lib.vgl_bgzf_host_submit(h, bufs[0], cap + 1, C.byref(x)) == _abi.VGL_E_ARG
        for i in (0, 1):
            rc, got = wait(t[i].value)
            assert rc == _abi.VGL_OK and got == _compress(_dev(inputs[i])), i
            _equal_to_model(got, inputs[i])
            assert wait(t[i].value)[0] == _abi.VGL_E_ARG                        # already waited
        for bad in (-1, 2, 7):
            assert wait(bad)[0] == _abi.VGL_E_ARG
        # n = 0: an empty batch
        assert lib.vgl_bgzf_host_submit(h, bufs[2], 0, C.byref(t[2])) == _abi.VGL_OK
        rc, got = wait(t[2].value)
        assert rc == _abi.VGL_OK and out_n.value == 0 and got == b""
    finally:
        assert lib.vgl_bgzf_host_destroy(h) == _abi.VGL_OK
