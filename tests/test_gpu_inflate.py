"""The device inflater through vcfgl_amd.bgzf.decompress / inflate_members: every member of the corpus (tests/inflate_corpus.py)
inflated to its exact bytes, the stream split at a member boundary, decompress(compress(t)), damaged members among good ones with
a guarded destination, and ranges outside the buffers refused before the decoder runs."""
import numpy as np
import pytest
import torch

import inflate_corpus as ic
from vcfgl_amd import _abi, bgzf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), np.uint8).copy()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    return t.cpu().numpy().tobytes()


def test_every_good_member_in_one_stream():
    good = ic.good()
    out, status = bgzf.decompress(dev(ic.stream([m for _, m, _ in good])))
    st = status.cpu().numpy()
    assert status.dtype == torch.int32 and out.device == status.device and out.device.type == "cuda"
    assert [n for (n, _, _), s in zip(good, st) if s != _abi.INFLATE_OK] == [] and len(st) == len(good)
    got, off = host(out), 0
    for name, _, data in good:
        assert got[off:off + len(data)] == data, name
        off += len(data)
    assert off == len(got)


def test_the_stream_split_at_a_member_boundary():
    good = ic.good()
    k = len(good) // 2
    whole = host(bgzf.decompress(dev(ic.stream([m for _, m, _ in good])))[0])
    a, sa = bgzf.decompress(dev(ic.stream([m for _, m, _ in good[:k]])))
    b, sb = bgzf.decompress(dev(ic.stream([m for _, m, _ in good[k:]])))
    assert int(sa.abs().sum()) == 0 and int(sb.abs().sum()) == 0
    assert host(a) + host(b) == whole == b"".join(d for _, _, d in good)


@pytest.mark.parametrize("what", ["text", "random"])
def test_decompress_of_compress(what):
    if what == "text":
        data = ic.vcf_text(3 * 0xff00 + 17)
    else:
        data = np.random.default_rng(1).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()     # stored members
    comp = bgzf.compress(dev(data))
    out, status = bgzf.decompress(comp)
    assert status.numel() == (len(data) + 0xff00 - 1) // 0xff00 and int(status.abs().sum()) == 0
    assert host(out) == data
    if what == "random":
        assert comp.numel() > len(data)
    out, status = bgzf.decompress(torch.cat([comp, dev(bgzf.EOF)]))                            # with the EOF member: one more, empty
    assert status.numel() == (len(data) + 0xff00 - 1) // 0xff00 + 1 and int(status.abs().sum()) == 0 and host(out) == data


GUARD, PATTERN = 4096, 0xA7


def test_damaged_members_among_good_ones_and_a_guarded_destination():
    good, bad = ic.good(), ic.damaged()
    members, want = [], []
    for i, (name, raw) in enumerate(bad):
        g = good[(3 * i) % len(good)]
        members += [raw, g[1]]; want += [None, g[2]]
    assert len(members) <= 40
    raw = ic.stream(members)
    begin, csize, isize = bgzf.index(raw)
    # outputs 37 bytes apart (every alignment of a member's first byte), a guard in front, between and behind
    out_off, at = [], GUARD
    for n in isize:
        out_off.append(at); at += int(n) + 37
    dst = torch.full((at + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    status = bgzf.inflate_members(dev(raw), dev(begin), dev(csize), dev(out_off, np.int64), dev(isize), dst).cpu().numpy()
    got = dst.cpu().numpy()
    covered = np.zeros(len(got), bool)
    for i, w in enumerate(want):
        lo, hi = out_off[i], out_off[i] + int(isize[i])
        covered[lo:hi] = True
        if w is None:
            assert status[i] == _abi.INFLATE_HOST, bad[i // 2][0]
        else:
            assert status[i] == _abi.INFLATE_OK and got[lo:hi].tobytes() == w, i
    assert (got[~covered] == PATTERN).all()


def test_ranges_outside_the_buffers_are_refused_and_nothing_is_written():
    good = ic.good()[:4]
    raw = ic.stream([m for _, m, _ in good])
    begin, csize, isize = bgzf.index(raw)
    out_off = np.concatenate([[0], np.cumsum(isize, dtype=np.int64)])[:-1]
    total = int(isize.sum())
    src = dev(raw)
    cases = {"negative begin": (1, "begin", -1), "isize 65537": (2, "isize", 65537), "csize past src_bytes": (3, "csize", int(csize[3]) + 1),
             "negative csize": (0, "csize", -5), "negative out_off": (0, "out_off", -1), "out_off past dst": (3, "out_off", int(out_off[3]) + 1),
             "begin past src_bytes": (2, "begin", len(raw) + 1), "negative isize": (1, "isize", -1)}
    for what, (k, field, value) in cases.items():
        arr = {"begin": begin.copy(), "csize": csize.copy(), "isize": isize.copy(), "out_off": out_off.copy()}
        arr[field][k] = value
        dst = torch.full((total,), PATTERN, dtype=torch.uint8, device=DEV)
        with pytest.raises(bgzf.BgzfArgError):
            bgzf.inflate_members(src, dev(arr["begin"]), dev(arr["csize"]), dev(arr["out_off"]), dev(arr["isize"]), dst)
        assert bool((dst == PATTERN).all()), what
    dst = torch.full((total,), PATTERN, dtype=torch.uint8, device=DEV)
    status = bgzf.inflate_members(src, dev(begin), dev(csize), dev(out_off), dev(isize), dst)
    assert int(status.abs().sum()) == 0 and host(dst) == b"".join(d for _, _, d in good)


def test_a_wrong_isize_or_a_range_that_is_not_a_member_is_left_to_the_host():
    """ranges inside the buffers that do not describe the member: HOST, and nothing outside [out_off, out_off + isize) is written"""
    name, raw, data = ic.good()[0]
    src = dev(raw + raw)
    begin = np.array([0, 0, 5, len(raw)], np.int64)
    csize = np.array([len(raw), len(raw) - 1, len(raw) - 5, len(raw)], np.int32)
    isize = np.array([len(data) - 1, len(data), len(data), len(data)], np.int32)
    out_off = GUARD + np.arange(4, dtype=np.int64) * 65536
    dst = torch.full((GUARD + 4 * 65536,), PATTERN, dtype=torch.uint8, device=DEV)
    status = bgzf.inflate_members(src, dev(begin), dev(csize), dev(out_off), dev(isize), dst).cpu().numpy()
    assert list(status) == [1, 1, 1, 0]
    got = dst.cpu().numpy()
    assert got[out_off[3]:out_off[3] + len(data)].tobytes() == data
    assert (got[:GUARD] == PATTERN).all() and (got[out_off[3] + len(data):] == PATTERN).all()
    for k in range(3):
        assert (got[out_off[k] + isize[k]:out_off[k + 1]] == PATTERN).all()


def test_host_batches_two_in_flight_and_a_third_refused():
    import ctypes as C
    lib = _abi.load_library()
    good = ic.good()
    h = C.c_void_p()
    assert lib.vgl_inflate_host_create(0, 16, C.byref(h)) == _abi.VGL_OK
    try:
        tickets, wants = [], []
        for part in (good[:9], good[9:]):
            raw = ic.stream([m for _, m, _ in part])
            begin, csize, isize = bgzf.index(raw)
            t = C.c_int32(-1)
            assert lib.vgl_inflate_host_submit(h, raw, len(raw), len(begin), begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(t)) == _abi.VGL_OK
            tickets.append(t.value); wants.append(b"".join(d for _, _, d in part))
        t = C.c_int32(-1)
        assert lib.vgl_inflate_host_submit(h, raw, len(raw), len(begin), begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(t)) == _abi.VGL_E_ARG
        assert b"two batches are in flight" in lib.vgl_last_error()
        bad = isize.copy(); bad[0] = 65537
        assert lib.vgl_inflate_host_submit(h, raw, len(raw), len(begin), begin.ctypes.data, csize.ctypes.data, bad.ctypes.data, C.byref(t)) == _abi.VGL_E_ARG
        assert lib.vgl_inflate_host_submit(h, raw, len(raw), 17, begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(t)) == _abi.VGL_E_ARG
        for ticket, want, n in zip(tickets, wants, (9, len(good) - 9)):
            out, out_n, status = C.c_void_p(), C.c_int64(), C.c_void_p()
            assert lib.vgl_inflate_host_wait(h, ticket, C.byref(out), C.byref(out_n), C.byref(status)) == _abi.VGL_OK
            assert out_n.value == len(want) and C.string_at(out.value, out_n.value) == want
            assert list((C.c_int32 * n).from_address(status.value)) == [0] * n
        assert lib.vgl_inflate_host_wait(h, tickets[0], C.byref(out), C.byref(out_n), C.byref(status)) == _abi.VGL_E_ARG
    finally:
        assert lib.vgl_inflate_host_destroy(h) == _abi.VGL_OK
