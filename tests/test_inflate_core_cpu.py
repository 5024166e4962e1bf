"""The inflater's decoder (vcfgl_amd/csrc/vgl_inflate_core.h) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program with its own main (tests/inflate_core_main.cpp) decodes every member of the corpus into allocations of exactly
the member's size and exactly ISIZE bytes.  Every member zlib or the compressor's model wrote must come back OK with zlib's bytes --
the host fallback of the product must not be able to hide a decoder that cannot decode -- and every damaged one HOST."""
import os
import struct
import subprocess
import zlib

import pytest

import inflate_corpus as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_core") / "inflate_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "inflate_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def decode(program, members, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for m in members:
            f.write(struct.pack("<I", len(m)) + m)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    raw, off, out = open(fout, "rb").read(), 0, []
    while off < len(raw):
        status, check, n = struct.unpack_from("<III", raw, off)
        out.append((status, check, raw[off + 12:off + 12 + n]))
        off += 12 + n
    assert off == len(raw) and len(out) == len(members)
    return out, r.stdout


def test_every_good_member_is_decoded(program, tmp_path):
    good = ic.good()
    assert len(good) >= 20
    got, stdout = decode(program, [raw for _, raw, _ in good], tmp_path)
    for (name, raw, data), (status, check, out) in zip(good, got):
        assert (status, check) == (0, 0), (name, status, check)
        assert out == data == zlib.decompress(ic.deflate_of(raw), -15), name
    assert stdout.split() == ["members", str(len(good)), "index", "0", str(len(good)), "cut_refused", "1"]


def test_every_damaged_member_is_refused(program, tmp_path):
    bad = ic.damaged()
    names = {n for n, _ in bad}
    assert {"bit_flip_in_the_huffman_data", "crc_flipped", "isize_plus_1", "isize_minus_1", "btype_11", "len_nlen_mismatch", "data_cut_short",
            "distance_before_the_start", "more_than_isize"} <= names
    got, stdout = decode(program, [raw for _, raw in bad], tmp_path)
    checks = {}
    for (name, raw), (status, check, out) in zip(bad, got):
        assert status == 1 and out == b"", (name, status, check)
        checks[name] = check
    # the check that refused it is the one the damage was made for
    assert checks["crc_flipped"] == 101 and checks["btype_11"] == 3 and checks["len_nlen_mismatch"] == 4 and checks["distance_before_the_start"] == 19
    assert checks["isize_plus_1"] == 20 and checks["isize_minus_1"] == 5 and checks["more_than_isize"] == 5 and checks["more_than_isize_stored"] == 5
    assert checks["stored_cut_short"] == 2 and checks["bytes_after_the_final_block"] == 21
    assert "index 0 %d " % len(bad) in stdout                          # damaged inside: the container of every one is whole


def test_good_and_damaged_interleaved(program, tmp_path):
    """the tables of one member are the next one's scratch: a refused member leaves nothing behind that the next decode uses"""
    good, bad = ic.good(), ic.damaged()
    members, want = [], []
    for i, (name, raw) in enumerate(bad):
        g = good[i % len(good)]
        members += [raw, g[1]]; want += [None, g[2]]
    got, _ = decode(program, members, tmp_path)
    for w, (status, check, out) in zip(want, got):
        assert (status == 1) if w is None else (status == 0 and out == w)
