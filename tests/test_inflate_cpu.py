"""BGZF input without a GPU: vgl_bgzf_index (pure host arithmetic) against bgzf_model.split_members, what it refuses, the
declarations of the inflater's entry points, and the refusals of vcfgl_hip --device-inflate."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bgzf_model as bm
import golden_util as gu
import inflate_corpus as ic
from vcfgl_amd import _abi, bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def raw_index(raw, cap=None):
    lib = _abi.load_library()
    cap = len(raw) // 28 + 1 if cap is None else cap
    begin, csize, isize = np.zeros(max(1, cap), np.int64), np.zeros(max(1, cap), np.int32), np.zeros(max(1, cap), np.int32)
    n = C.c_int64(-7)
    buf = (C.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0")
    rc = lib.vgl_bgzf_index(buf, len(raw), cap, begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(n))
    return rc, n.value, begin, csize, isize


def test_index_equals_the_model_split():
    good = ic.good()
    raw = ic.stream([m for _, m, _ in good] + [m for _, m in ic.damaged()])
    members = bm_split(raw)
    rc, n, begin, csize, isize = raw_index(raw)
    assert rc == _abi.VGL_OK and n == len(members) == len(good) + len(ic.damaged())
    off = 0
    for i, m in enumerate(members):
        assert (begin[i], csize[i]) == (off, len(m)) and isize[i] == struct.unpack_from("<I", m, len(m) - 4)[0], i
        off += len(m)
    for (name, m, data), k in zip(good, isize):
        assert k == len(data), name
    names = [g[0] for g in good]
    assert csize[names.index("eof")] == 28 and isize[names.index("eof")] == 0       # the EOF member counts like any other
    b2, c2, i2 = bgzf.index(raw)
    assert np.array_equal(b2, begin[:n]) and np.array_equal(c2, csize[:n]) and np.array_equal(i2, isize[:n])


def bm_split(raw):
    """bgzf_model.split_members reads BSIZE at byte 16: the member with a subfield in front of 'BC' is split by hand"""
    out, off = [], 0
    while off < len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        if xlen == 6:
            m = bm.split_members(raw[off:off + struct.unpack_from("<H", raw, off + 16)[0] + 1])[0]
        else:
            at = raw.index(b"BC\x02\x00", off + 12)
            assert at < off + 12 + xlen
            m = raw[off:off + struct.unpack_from("<H", raw, at + 4)[0] + 1]
        out.append(m); off += len(m)
    assert off == len(raw)
    return out


def test_index_of_the_model_stream_equals_split_members():
    data = ic.vcf_text(2 * bm.MEMBER + 17)
    raw = b"".join(ic.wrap(ic.deflate(data[i:i + bm.MEMBER]), data[i:i + bm.MEMBER]) for i in range(0, len(data), bm.MEMBER)) + ic.EOF
    members = bm.split_members(raw)
    rc, n, begin, csize, isize = raw_index(raw)
    assert rc == _abi.VGL_OK and n == len(members) == 4
    assert list(csize[:n]) == [len(m) for m in members] and list(begin[:n]) == list(np.cumsum([0] + [len(m) for m in members[:-1]]))
    assert list(isize[:n]) == [bm.MEMBER, bm.MEMBER, 17, 0]


def test_index_refuses_what_is_not_a_clean_series_of_members():
    lib = _abi.load_library()
    good = ic.stream([m for _, m, _ in ic.good()[:5]])
    text = ic.vcf_text(5000)
    for what, raw in (("plain text", text), ("gzip", gzip.compress(text)), ("cut inside the last member", good[:-1]), ("cut in the last trailer", good[:-5]),
                      ("cut in the last header", good[:len(good) - len(ic.good()[4][1]) + 7]), ("trailing bytes", good + b"\n"),
                      ("trailing gzip member", good + gzip.compress(b"x")), ("empty", b""), ("gzip first", gzip.compress(text) + good)):
        rc, n, *_ = raw_index(raw)
        assert rc == _abi.VGL_E_UNSUPPORTED and n == 0, what
        assert b"vgl_bgzf_index" in lib.vgl_last_error()
        with pytest.raises(ValueError):
            bgzf.index(raw)
    big = ic.wrap(ic.deflate(bytes(70000)), bytes(70000))                 # a gzip member in BGZF's clothes: ISIZE > 65536
    assert raw_index(big)[0] == _abi.VGL_E_UNSUPPORTED
    nobc = bytearray(ic.good()[0][1]); nobc[12:14] = b"XY"
    assert raw_index(bytes(nobc))[0] == _abi.VGL_E_UNSUPPORTED
    flg = bytearray(ic.good()[0][1]); flg[3] = 0
    assert raw_index(bytes(flg))[0] == _abi.VGL_E_UNSUPPORTED


def test_index_arguments():
    lib = _abi.load_library()
    raw = ic.stream([m for _, m, _ in ic.good()[:3]])
    rc, n, *_ = raw_index(raw, cap=2)
    assert rc == _abi.VGL_E_CAPACITY and n == 3
    rc, n, begin, csize, isize = raw_index(raw, cap=3)
    assert rc == _abi.VGL_OK and n == 3
    k = C.c_int64()
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    assert lib.vgl_bgzf_index(buf, len(raw), 3, None, None, None, C.byref(k)) == _abi.VGL_E_ARG
    assert lib.vgl_bgzf_index(buf, len(raw), 3, begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, None) == _abi.VGL_E_ARG
    assert lib.vgl_bgzf_index(None, 0, 0, None, None, None, C.byref(k)) == _abi.VGL_E_ARG
    assert lib.vgl_bgzf_index(buf, len(raw), 0, None, None, None, C.byref(k)) == _abi.VGL_E_CAPACITY and k.value == 3     # counting


NEW = ["vgl_bgzf_index", "vgl_inflate_workspace_bytes", "vgl_inflate_members_device", "vgl_inflate_host_create", "vgl_inflate_host_submit",
       "vgl_inflate_host_wait", "vgl_inflate_host_destroy"]


def test_declarations():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define\s+VGL_ABI_VERSION\s+7\b", hdr) and _abi.ABI_VERSION == 7
    assert re.search(r"#define\s+VGL_INFLATE_OK\s+0\b", hdr) and re.search(r"#define\s+VGL_INFLATE_HOST\s+1\b", hdr)
    assert (_abi.INFLATE_OK, _abi.INFLATE_HOST) == (0, 1)
    for lib in (_abi.load_library(), _abi.load_library(hooks=True)):
        for name in NEW:
            assert re.search(r"VGL_API\s+\w+\s+%s\(" % name, hdr), name
            assert name in _abi.EXPORTS and getattr(lib, name).argtypes, name
        assert lib.vgl_inflate_workspace_bytes(512) > 0 and lib.vgl_inflate_workspace_bytes(-1) == -1
    assert callable(bgzf.decompress) and callable(bgzf.index)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_inflate_host_create(0, 0, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_inflate_host_create(0, 512, None) == _abi.VGL_E_ARG
    assert lib.vgl_inflate_host_destroy(None) == _abi.VGL_OK
    assert lib.vgl_inflate_members_device(0, None, 10, 1, None, None, None, None, None, 10, None, None, 0, None) == _abi.VGL_E_ARG
    assert lib.vgl_inflate_members_device(0, None, -1, 0, None, None, None, None, None, 0, None, None, 0, None) == _abi.VGL_E_ARG
    assert lib.vgl_inflate_host_submit(None, None, 0, 0, None, None, None, None) == _abi.VGL_E_ARG
    assert lib.vgl_inflate_host_wait(None, 0, None, None, None) == _abi.VGL_E_ARG


@pytest.mark.skipif(_have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_entry_points_are_refused():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_inflate_host_create(0, 512, C.byref(h)) == _abi.VGL_E_NODEVICE
    assert not h.value and b"vgl_inflate_host_create" in lib.vgl_last_error()
    buf = (C.c_uint8 * 256)()                                          # (never touched: the device count is asked first)
    p = C.addressof(buf)
    assert lib.vgl_inflate_members_device(0, p, 16, 1, p, p, p, p, p, 16, p, p, 256, None) == _abi.VGL_E_NODEVICE
    assert b"vgl_inflate_members_device" in lib.vgl_last_error()


ARGV = ["-i", os.path.join(gu.REFVCF, "data", "data2.vcf"), "--seed", "1", "-e", "0.01", "-O", "v"]


def test_bad_values_and_depth_inf_are_refused_and_nothing_is_written(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN] + ARGV + ["-o", out, "--depth", "inf", "--device-inflate", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-inflate 1 is not supported with --depth inf" in r.stderr
    assert os.listdir(str(tmp_path)) == []
    for v in ("2", "-1"):
        r = subprocess.run([BIN] + ARGV + ["-o", out, "--depth", "1", "--device-inflate", v], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--device-inflate" in r.stderr and os.listdir(str(tmp_path)) == []
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert "--device-inflate 0|1" in r.stderr


@pytest.mark.skipif(_have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_program_fails_instead_of_falling_back(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN] + ARGV + ["-o", out, "--depth", "1", "--device-inflate", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-inflate 1:" in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith((".vcf", ".bcf", ".gz"))]
