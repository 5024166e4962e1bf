"""The device inflater (k_inflate_member) on deflate streams that zlib's compressor never writes: the members of
tests/inflate_shapes.py -- shaped(), refused(), fuzzed() -- through bgzf.inflate_members into a guarded destination, every size
edge at every destination alignment, the staging limit, the record loop's entry points, and vcfgl_hip --device-inflate 1 on a file
the builder wrote.  The CPU side of the same cases is test_inflate_shapes_cpu.py; what only the device has -- 64 lanes sharing
match copies, the staging, the write-out, the CRC32 slices -- is held here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import inflate_corpus as ic
import inflate_shapes as sh
import test_gpu_cli_inflate as tgi
from vcfgl_amd import _abi, bgzf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN, GAP = 4096, 0xA7, 37
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype=None):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), np.uint8).copy()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def inflate_guarded(members, out_off=None, dst=None):
    """one launch over `members` (bytes each) into a destination filled with a pattern: (statuses, [the bytes at each member's
    range]).  Outputs lie GAP bytes apart (every alignment of a member's first byte) behind a guard unless out_off and dst (filled
    with the pattern) say where; asserts that no byte outside the members' ranges changed."""
    raw = ic.stream(members)
    begin, csize, isize = bgzf.index(raw)
    assert len(begin) == len(members)
    if out_off is None:
        out_off, at = [], GUARD
        for n in isize:
            out_off.append(at); at += int(n) + GAP
        dst = torch.full((at + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    status = bgzf.inflate_members(dev(raw), dev(begin), dev(csize), dev(out_off, np.int64), dev(isize), dst).cpu().numpy()
    got = dst.cpu().numpy()
    covered = np.zeros(len(got), bool)
    outs = []
    for i in range(len(members)):
        lo, hi = int(out_off[i]), int(out_off[i]) + int(isize[i])
        covered[lo:hi] = True
        outs.append(got[lo:hi].tobytes())
    untouched = got[~covered] == PATTERN
    assert untouched.all(), "bytes outside every member's range were written, first at %d" % int(np.flatnonzero(~covered)[np.argmin(untouched)])
    return status, outs


def assert_verdicts(names, want, status, outs):
    """want[i]: the bytes of an OK member, None for HOST"""
    wrong = []
    for name, w, s, o in zip(names, want, status, outs):
        if w is None:
            if s != _abi.INFLATE_HOST:
                wrong.append((name, "accepted, must be refused"))
        elif s != _abi.INFLATE_OK:
            wrong.append((name, "refused (status %d), must be decoded" % s))
        elif o != w:
            wrong.append((name, "wrong bytes, first at %d of %d" % (next(i for i in range(len(w)) if o[i] != w[i]), len(w))))
    assert wrong == [], wrong[:20]


@pytest.fixture(scope="module")
def shaped_on_the_device():
    good = sh.shaped()
    status, outs = inflate_guarded([m for _, m, _ in good])
    return good, status, outs


def test_shaped_and_refused_members(shaped_on_the_device):
    good, status, outs = shaped_on_the_device
    assert_verdicts([n for n, _, _ in good], [d for _, _, d in good], status, outs)
    bad = sh.refused()
    members, names, want = [], [], []
    for i, (name, m, _) in enumerate(bad):               # refused members among good ones
        g = good[(5 * i) % len(good)]
        members += [m, g[1]]; names += [name, g[0]]; want += [None, g[2]]
    status, outs = inflate_guarded(members)
    assert_verdicts(names, want, status, outs)


def test_fuzzed_streams_and_one_bit_mutants():
    streams, mutants = sh.fuzzed()
    assert len(streams) == 500 and len(mutants) == 2000
    status, outs = inflate_guarded([m for _, m, _ in streams])
    assert_verdicts([n for n, _, _ in streams], [d for _, _, d in streams], status, outs)
    status, outs = inflate_guarded([m for _, m, _ in mutants])
    assert_verdicts([n for n, _, _ in mutants], [w for _, _, w in mutants], status, outs)


def test_every_size_edge_at_every_destination_alignment():
    by_size = {len(d): (m, d) for n, m, d in sh.shaped() if "isize_" in n}
    assert sorted(by_size) == sorted(sh.SIZE_EDGES) and len(sh.SIZE_EDGES) == 17
    cases = [(n, a) for n in sh.SIZE_EDGES for a in range(16)]
    dst = torch.full((GUARD + sum(n + 64 for n, _ in cases) + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    ptr = dst.data_ptr()
    members, want, out_off, at = [], [], [], GUARD
    for n, a in cases:
        at += 17                                         # at least 17 guard bytes in front of every output
        at += (a - (ptr + at)) % 16
        out_off.append(at); members.append(by_size[n][0]); want.append(by_size[n][1])
        at += n
    assert at + GUARD <= dst.numel()
    status, outs = inflate_guarded(members, out_off=out_off, dst=dst)
    assert {((ptr + o) % 16, len(w)) for o, w in zip(out_off, want)} == {(a, n) for n, a in cases} and len(cases) == 17 * 16
    assert_verdicts(["isize %d at alignment %d" % c for c in cases], want, status, outs)


def test_the_staging_limit(shaped_on_the_device):
    src = open(os.path.join(ROOT, "vcfgl_amd", "csrc", "vgl_inflate.hip")).read()
    (in_lds,) = re.findall(r"^constexpr int IN_LDS = (\d+);", src, re.M)
    in_lds = int(in_lds)
    assert re.search(r"if \(in_len <= IN_LDS\)", src)
    lens = sh.staging_in_lens()
    assert {in_lds - 1, in_lds, in_lds + 1} <= set(lens.values()) and {n % 4 for n in lens.values() if n > in_lds} == {0, 1, 2, 3}
    good, status, outs = shaped_on_the_device
    pick = [i for i, (n, _, _) in enumerate(good) if n in lens]
    assert len(pick) == 6
    # in a launch of their own as well, at the destination's first bytes
    status2, outs2 = inflate_guarded([good[i][1] for i in pick])
    for st, ou in ((status[pick], [outs[i] for i in pick]), (status2, outs2)):
        assert_verdicts([good[i][0] for i in pick], [good[i][2] for i in pick], st, ou)


def test_the_record_loops_entry_gives_what_the_stateless_entry_gives(shaped_on_the_device):
    good, status, outs = shaped_on_the_device
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_inflate_host_create(0, 16, C.byref(h)) == _abi.VGL_OK
    got_status, got_outs = [], []

    def wait(ticket, part):
        out, out_n, st = C.c_void_p(), C.c_int64(), C.c_void_p()
        assert lib.vgl_inflate_host_wait(h, ticket, C.byref(out), C.byref(out_n), C.byref(st)) == _abi.VGL_OK
        assert out_n.value == sum(len(d) for _, _, d in part)
        raw, off = C.string_at(out.value, out_n.value), 0
        for _, _, d in part:
            got_outs.append(raw[off:off + len(d)]); off += len(d)
        got_status.extend((C.c_int32 * len(part)).from_address(st.value))
    try:
        pending = []
        for k in range(0, len(good), 16):                # two batches in flight: batch b is submitted before b - 1 is waited for
            part = good[k:k + 16]
            raw = ic.stream([m for _, m, _ in part])
            begin, csize, isize = bgzf.index(raw)
            t = C.c_int32(-1)
            assert lib.vgl_inflate_host_submit(h, raw, len(raw), len(begin), begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(t)) == _abi.VGL_OK
            pending.append((t.value, part))
            if len(pending) == 2:
                wait(*pending.pop(0))
        while pending:
            wait(*pending.pop(0))
    finally:
        assert lib.vgl_inflate_host_destroy(h) == _abi.VGL_OK
    assert len(good) > 5 * 16 and got_status == [int(s) for s in status] == [0] * len(good)
    assert got_outs == outs == [d for _, _, d in good]


FLAGS = "--seed 42 --depth 4 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -addPL 1 -O v --tile-sites 256 --verbose 1".split()


def test_the_host_program_on_a_file_the_builder_wrote(tmp_path):
    """300 lines x 50 samples in members of 1 .. 3 KiB: stored, fixed, dynamic with 15-bit codes, several blocks, in turn"""
    data = sh.vcf_for_the_host_program(300, 50)
    raw, n_members = sh.bgzf_by_builder(data, seed=3)
    assert n_members > 25
    path = str(tmp_path / "in.vcf.gz")
    open(path, "wb").write(raw)
    res = {}
    for k, extra in (("0", ["--device-inflate", "0"]), ("1", ["--device-inflate", "1", "--device-input", "0"]), ("2", ["--device-inflate", "1", "--device-input", "1"])):
        res[k] = tgi.run(["-i", path, "-o", str(tmp_path / ("o" + k))] + FLAGS + extra)
    assert tgi.same_outputs("o0", "o1", tmp_path) == tgi.same_outputs("o0", "o2", tmp_path) == [".vcf"]
    assert res["0"].stdout == res["1"].stdout == res["2"].stdout
    for k in ("1", "2"):
        m = tgi.INFLATED.search(res[k].stderr)          # every member on the device, no fallback: zlib never read the file
        assert m and int(m.group(1)) == n_members and int(m.group(2)) == len(raw) and int(m.group(3)) == len(data), res[k].stderr[-1500:]
        assert not tgi.FELL_BACK.search(res[k].stderr)
    assert tgi.tci.input_line(res["2"].stderr) == (300, 0)
