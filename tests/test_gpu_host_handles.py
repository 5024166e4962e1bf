"""The five host-batch families (vgl_bgzf_host_*, vgl_stream_host_*, vgl_vcfin_host_*, vgl_inflate_host_*, vgl_bcfin_host_*;
vcfgl_amd/csrc/hostlib/batch.h) give back what they took and destroy cleanly with a batch in flight.

Memory: per family five cycles of create, two tiny batches submitted and then waited for (both slots in flight), destroy, and the
free device memory (torch.cuda.mem_get_info) after each destroy.  Cycle 1 warms the runtime; the drift is what cycles 3 .. 5 lose
against the reading after cycle 2, and it stays below PARENT_DRIFT + GRANULE.  GRANULE = 2097152 is what
tests/test_gpu_ctx_lifecycle.py measured: the reading moves in chunks of 2 MiB, so this guards the large buffers -- the capacities
are chosen so that the slot buffers exceed the granule (inflate: 64 members, 4 MiB each way; vcfin / bcfin: 8 MiB of text or GT
bytes, 2000 lines; bgzf: batches of 4 MiB; stream: two buffers with 4 MiB of heads and of bodies) -- and is no proof of no leak:
the results' staging of vcfin / bcfin at 8 samples (32 KB) and the words of sizes are below it.  The owners' own guard is
tests/test_hostbatch_cpu.py, under the leak checker.  The batches are the smallest that use both slots: 8 samples; 16 lines or
records, one of which the device hands back; 4 BGZF members, one of them empty; 0xff00 + 1 bytes to compress (two members); 8 sites.

Recorded on 5af6def (the last commit whose handles freed by hand in the kernel files; VGL_LIB selects that build), one MI355X,
free bytes after each of the five destroys (profiles/host_batch_ab/handles_on_parent.log):
    bgzf     308396687360 308394590208 308394590208 308394590208 308394590208
    stream   308384104448 308384104448 308384104448 308384104448 308384104448
    vcfin    308382007296 308382007296 308382007296 308382007296 308382007296
    inflate  308379910144 308379910144 308379910144 308379910144 308379910144
    bcfin    308377812992 308377812992 308377812992 308377812992 308377812992
so PARENT_DRIFT = 0 bytes (this build: the same twenty-five numbers).

Destroy with a batch in flight: submit, no wait, *_host_destroy returns VGL_OK (it waits for the handle's streams); a fresh handle
of the family then returns, for the same batch, what the family's CPU model or zlib gives."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import bcfin_cases as bc
import bgzf_model
import inflate_corpus as ic
import stream_model as sm
import vcfin_cases as vc
from vcfgl_amd import _abi, bgzf

pytestmark = pytest.mark.gpu
CYCLES = 5
PARENT_DRIFT = 0
GRANULE = 2097152
N = 8
MIB = 1 << 20
FAMILIES = ["bgzf", "stream", "vcfin", "inflate", "bcfin"]


def ok(lib, rc):
    assert rc == _abi.VGL_OK, lib.vgl_last_error()


def rows_sums_status(lib, wait, h, ticket, n):
    g, s, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(lib, wait(h, ticket, C.byref(g), C.byref(s), C.byref(st)))
    return (np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=(n * N,)).reshape(n, N).copy(),
            np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(n,)).copy(),
            np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_int32)), shape=(n,)).copy())


def same_rows(got, case):
    rows, sums, status = case.expected()
    good = status == 0
    return (np.array_equal(got[2], status) and int(status.sum()) == 1 and np.array_equal(got[0][good], rows[good])
            and np.array_equal(got[1][good], sums[good]))


def members_inflate_to(members, data):
    """every member's header size, CRC32 and ISIZE, and zlib's inflate of its deflate data"""
    parts = bgzf_model.split_members(members)
    for g in parts:
        piece = zlib.decompress(g[18:-8], -15)
        assert int.from_bytes(g[-8:-4], "little") == zlib.crc32(piece) and int.from_bytes(g[-4:], "little") == len(piece)
    return b"".join(zlib.decompress(g[18:-8], -15) for g in parts) == bytes(data)


class Bgzf:
    """two batches of 0xff00 + 1 bytes: two members each"""
    def __init__(self):
        self.lib = _abi.load_library()
        rng = np.random.default_rng(21)
        words = [b"0/1", b"1/1", b"\t", b"PASS", b"-0.5", b"\n"]
        text = b"".join(words[i] for i in rng.integers(0, len(words), 60000))
        self.data = [text[:bgzf_model.MEMBER + 1], text[5:5 + bgzf_model.MEMBER + 1]]
        self.bufs = [C.create_string_buffer(x, len(x)) for x in self.data]

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_bgzf_host_create(0, 4 * MIB, C.byref(h)))
        return h

    def submit(self, h, k):
        t = C.c_int32(-1)
        ok(self.lib, self.lib.vgl_bgzf_host_submit(h, self.bufs[k], len(self.data[k]), C.byref(t)))
        return t.value

    def wait(self, h, ticket, k):
        out, n = C.c_void_p(), C.c_int64()
        ok(self.lib, self.lib.vgl_bgzf_host_wait(h, ticket, C.byref(out), C.byref(n)))
        return C.string_at(out.value, n.value)

    def right(self, got, k):
        return len(bgzf_model.split_members(got)) == 2 and members_inflate_to(got, self.data[k])

    def destroy(self, h):
        return self.lib.vgl_bgzf_host_destroy(h)


class Stream:
    """two tiles of 8 sites, one per buffer"""
    def __init__(self):
        self.lib = _abi.load_library()
        rng = np.random.default_rng(22)
        self.tiles = []
        for _ in range(2):
            hl, bl = rng.integers(20, 40, 8), rng.integers(0, 200, 8)
            off = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int64)
            self.tiles.append((rng.integers(0, 256, int(hl.sum()), dtype=np.uint8), off(hl), rng.integers(0, 4, int(bl.sum()), dtype=np.uint8), off(bl)))
        self.want = [bytes(sm.assemble(*t)[0]) for t in self.tiles]

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_stream_host_create(0, 2, 8, 4 * MIB, 4 * MIB, C.byref(h)))
        return h

    def submit(self, h, k):
        heads, ho, bodies, bo = self.tiles[k]
        # the bodies into buffer k: a one-site stream with no head, assembled at the buffer's address
        t = torch.from_numpy(bodies).cuda()
        z = torch.zeros(2, dtype=torch.int64, device="cuda")
        off = torch.tensor([0, t.numel()], dtype=torch.int64, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        body = self.lib.vgl_stream_host_body(h, k)
        assert body
        ok(self.lib, self.lib.vgl_stream_assemble_device(0, 1, t.data_ptr(), z.data_ptr(), t.data_ptr(), off.data_ptr(), body, t.numel(),
                                                         total.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ticket = C.c_int32(-1)
        ok(self.lib, self.lib.vgl_stream_host_submit(h, k, 8, heads.ctypes.data, ho.ctypes.data, bo.ctypes.data, C.byref(ticket)))
        return ticket.value

    def wait(self, h, ticket, k):
        p, n, raw = C.c_void_p(), C.c_int64(), C.c_int64()
        ok(self.lib, self.lib.vgl_stream_host_wait(h, ticket, C.byref(p), C.byref(n), C.byref(raw)))
        return C.string_at(p.value, n.value), raw.value

    def right(self, got, k):
        members, raw = got
        return raw == len(self.want[k]) and members == bgzf_model.compress(self.want[k]) and members_inflate_to(members, self.want[k])

    def destroy(self, h):
        return self.lib.vgl_stream_host_destroy(h)


class Vcfin:
    """two batches of 16 lines of 8 samples; line 5 of each has a token outside the grammar"""
    def __init__(self):
        self.lib = _abi.load_library()
        self.cases = []
        for k in range(2):
            rng = np.random.default_rng(23 + k)
            c = vc.Case(N)
            for i in range(16):
                if i == 5:
                    c.add([b"0|1"] * (N - 1) + [b"0|x"], fallback=True)
                else:
                    vc.random_line(c, rng)
            self.cases.append(c)

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_vcfin_host_create(0, N, 2000, 8 * MIB, C.byref(h)))
        return h

    def submit(self, h, k):
        text, *arrs = self.cases[k].arrays()
        arrs = [np.ascontiguousarray(x) for x in arrs]
        t = C.c_int32(-1)
        ok(self.lib, self.lib.vgl_vcfin_host_submit(h, text, len(text), 16, *[x.ctypes.data for x in arrs], C.byref(t)))
        return t.value

    def wait(self, h, ticket, k):
        return rows_sums_status(self.lib, self.lib.vgl_vcfin_host_wait, h, ticket, 16)

    def right(self, got, k):
        return same_rows(got, self.cases[k])

    def destroy(self, h):
        return self.lib.vgl_vcfin_host_destroy(h)


class Bcfin:
    """two batches of 16 records of 8 samples (int8, int16 and int32 vectors); record 5 of each holds the missing sentinel"""
    def __init__(self):
        self.lib = _abi.load_library()
        self.cases = []
        for k in range(2):
            rng = np.random.default_rng(25 + k)
            c = bc.Case(N)
            for i in range(16):
                c.pad(int(rng.integers(0, 9)))
                if i == 5:
                    c.add([[bc.gt_value(0), "M"]] * N, fallback=True)
                else:
                    bc.random_record(c, rng, gt_type=1 + i % 3, n=1 + i % 4)
            self.cases.append(c)

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_bcfin_host_create(0, N, 2000, 8 * MIB, C.byref(h)))
        return h

    def submit(self, h, k):
        data, *arrs = self.cases[k].arrays()
        arrs = [np.ascontiguousarray(x) for x in arrs]
        t = C.c_int32(-1)
        ok(self.lib, self.lib.vgl_bcfin_host_submit(h, data, len(data), 16, *[x.ctypes.data for x in arrs], C.byref(t)))
        return t.value

    def wait(self, h, ticket, k):
        return rows_sums_status(self.lib, self.lib.vgl_bcfin_host_wait, h, ticket, 16)

    def right(self, got, k):
        return same_rows(got, self.cases[k])

    def destroy(self, h):
        return self.lib.vgl_bcfin_host_destroy(h)


class Inflate:
    """two batches of 4 members at zlib level 6; the third of each is empty"""
    def __init__(self):
        self.lib = _abi.load_library()
        self.data, self.raw, self.index = [], [], []
        for k in range(2):
            text = ic.vcf_text(3000 + 7 * k, samples=N, seed=27 + k)
            pieces = [text[:1000], text[1000:1001], b"", text[1001:]]
            members = [ic.wrap(ic.deflate(p), p) for p in pieces]
            assert all(zlib.decompress(ic.deflate_of(m), -15) == p for m, p in zip(members, pieces))
            raw = b"".join(members)
            begin, csize, isize = bgzf.index(raw)
            assert list(isize) == [len(p) for p in pieces]
            self.data.append(text); self.raw.append(raw); self.index.append((begin, csize, isize))

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_inflate_host_create(0, 64, C.byref(h)))
        return h

    def submit(self, h, k):
        t = C.c_int32(-1)
        ok(self.lib, self.lib.vgl_inflate_host_submit(h, self.raw[k], len(self.raw[k]), 4, *[x.ctypes.data for x in self.index[k]], C.byref(t)))
        return t.value

    def wait(self, h, ticket, k):
        out, n, st = C.c_void_p(), C.c_int64(), C.c_void_p()
        ok(self.lib, self.lib.vgl_inflate_host_wait(h, ticket, C.byref(out), C.byref(n), C.byref(st)))
        return C.string_at(out.value, n.value), list((C.c_int32 * 4).from_address(st.value))

    def right(self, got, k):
        return got == (self.data[k], [0, 0, 0, 0])

    def destroy(self, h):
        return self.lib.vgl_inflate_host_destroy(h)


@functools.lru_cache(maxsize=None)
def family(name):
    return {"bgzf": Bgzf, "stream": Stream, "vcfin": Vcfin, "inflate": Inflate, "bcfin": Bcfin}[name]()


def one_cycle(f):
    h = f.create()
    tickets = [f.submit(h, 0), f.submit(h, 1)]
    got = [f.wait(h, tickets[k], k) for k in (0, 1)]
    assert f.right(got[0], 0) and f.right(got[1], 1)
    assert f.destroy(h) == _abi.VGL_OK
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("name", FAMILIES)
def test_five_cycles_give_the_memory_back(name):
    f = family(name)
    free = [one_cycle(f) for _ in range(CYCLES)]
    drift = free[1] - free[CYCLES - 1]
    print(f"{name}: free device memory after each destroy:", free, "drift from cycle 2 to cycle 5:", drift, "bytes")
    assert drift < PARENT_DRIFT + GRANULE


@pytest.mark.parametrize("name", FAMILIES)
def test_destroy_with_a_batch_in_flight(name):
    f = family(name)
    h = f.create()
    f.submit(h, 0)
    assert f.destroy(h) == _abi.VGL_OK                                    # (no wait: the slot is busy)
    torch.cuda.synchronize()
    again = f.create()
    try:
        assert f.right(f.wait(again, f.submit(again, 0), 0), 0)
    finally:
        assert f.destroy(again) == _abi.VGL_OK
