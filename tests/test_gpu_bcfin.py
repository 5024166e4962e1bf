"""k_bcfin_decode (vgl_bcfin.hip) against tests/bcfin_model.py, exact equality: the record sets of tests/bcfin_cases.py (sample counts
around the eight-sample step and the wavefront, record counts around the four records of a workgroup, int8 / int16 / int32 with one
to four values per sample, slices at every alignment, every kind of record outside the plain rule between plain neighbours), guard
bands around the three outputs, the argument checks, the Python wrapper and the host object."""
import ctypes as C

import numpy as np
import pytest
import torch

import bcfin_cases as bc
import bcfin_model as bm
from vcfgl_amd import _abi, bcfin

pytestmark = pytest.mark.gpu
GUARD = 64


def _guarded(n_bytes, dev):
    """a device buffer of n_bytes between two guard bands of 0xA5 (the payload starts on a 64-byte boundary)"""
    buf = torch.full((GUARD + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n_bytes]


def _intact(buf, n_bytes):
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == 0xA5).all() and (h[GUARD + n_bytes:] == 0xA5).all())


def _launch(arrays, N, shift=0):
    """the entry point on (bytes, begin, type, n, nal, amap), outputs between guard bands; returns rc and the buffers"""
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    data, begin, gt_type, n, nal, amap = arrays
    R = len(begin)
    b_all = torch.zeros(shift + len(data), dtype=torch.uint8, device=dev)
    b_all[shift:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_bytes = b_all[shift:]
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (begin, gt_type, n, nal, amap)]
    bufs = [_guarded(R * N, dev), _guarded(R * 4, dev), _guarded(R * 4, dev)]
    ws = torch.zeros(int(lib.vgl_bcfin_workspace_bytes(N, R)), dtype=torch.uint8, device=dev)
    rc = lib.vgl_bcfin_decode_device(0, d_bytes.data_ptr(), len(data), R, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                     d[4].data_ptr(), N, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, bufs, (b_all, d, ws)


def run_device(case, shift=0):
    """shift moves the bytes against the allocation's alignment"""
    lib = _abi.load_library()
    R, N = len(case.begin), case.N
    rc, ((g_buf, g), (s_buf, s), (st_buf, st)), _keep = _launch(case.arrays(), N, shift)
    assert rc == _abi.VGL_OK, lib.vgl_last_error()
    assert _intact(g_buf, R * N) and _intact(s_buf, R * 4) and _intact(st_buf, R * 4)
    return (g.cpu().numpy().reshape(R, N), s.cpu().numpy().view(np.int32), st.cpu().numpy().view(np.int32))


def check(case, **kw):
    rows, sums, status = case.expected()
    got_rows, got_sums, got_status = run_device(case, **kw)
    assert np.array_equal(got_status, status)
    ok = status == bm.BCFIN_OK
    assert {int(i) for i in np.nonzero(~ok)[0]} == case.fallback          # exactly the constructed records are handed back
    assert np.array_equal(got_sums[ok], sums[ok])
    assert np.array_equal(got_rows[ok], rows[ok])
    return got_rows, got_sums, got_status


@pytest.mark.parametrize("n", bc.SAMPLE_COUNTS)
def test_sample_counts(n):
    check(bc.case_samples(n))
    check(bc.case_samples(n), shift=5)


@pytest.mark.parametrize("n_records", bc.RECORD_COUNTS)
def test_record_counts(n_records):
    check(bc.case_records(n_records))


@pytest.mark.parametrize("gt_type,n", bc.TYPES_AND_N)
def test_types_and_values_per_sample(gt_type, n):
    check(bc.case_types(gt_type, n))


def test_slices_at_every_alignment():
    c = bc.case_align()
    check(c)
    check(c, shift=5)                                                     # and with the bytes themselves off the 16-byte boundaries


def test_records_outside_the_rule_are_handed_back_and_their_neighbours_are_intact():
    c = bc.case_fallback()
    rows, sums, status = check(c)
    assert status.sum() == len(bc.FALLBACK_KINDS) and status[0] == status[-1] == bm.BCFIN_OK
    check(c, shift=5)


def test_edges_inside_the_rule_are_decoded():
    rows, sums, status = check(bc.case_plain_edges())
    assert not status.any()


def test_records_the_five_entry_map_cannot_describe_are_handed_back():
    """n_alleles 0 and 6 through the C ABI: the caller's records, whatever their values"""
    c = bc.Case(66)
    vals = [[bc.gt_value(0), bc.gt_value(1, 1)]] * 66
    c.add(vals).add(vals, nal=6, fallback=True).add(vals, nal=0, fallback=True).add(vals, nal=5)
    rows, sums, status = check(c)
    assert list(status) == [0, 1, 1, 0] and np.array_equal(rows[0], rows[3]) and sums[0] == 66


def test_python_wrapper():
    c = bc.case_samples(513)
    data, begin, gt_type, n, nal, amap = c.arrays()
    dev = torch.device("cuda", 0)
    t = [torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)] + [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (begin, gt_type, n, nal, amap)]
    gt, sums, status = bcfin.decode_gt(*t, c.N, device=0)
    rows, want_sums, want_status = c.expected()
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (len(begin), c.N) and sums.dtype == status.dtype == torch.int32
    assert np.array_equal(gt.cpu().numpy(), rows) and np.array_equal(sums.cpu().numpy(), want_sums) and not status.cpu().numpy().any()
    with pytest.raises(ValueError):
        bcfin.decode_gt(t[0], t[1].to(torch.int32), *t[2:], c.N)
    with pytest.raises(ValueError):                                       # a slice that ends behind the bytes
        bcfin.decode_gt(t[0], t[1] + 1000, *t[2:], c.N)


def test_slices_outside_the_bytes_are_refused_and_nothing_is_launched():
    lib = _abi.load_library()
    c = bc.case_samples(64)
    data, begin, gt_type, n, nal, amap = c.arrays()
    for what in ("end beyond the bytes", "one byte beyond", "negative begin", "n beyond the bytes", "a huge n"):
        b2, n2 = begin.copy(), n.copy()
        if what == "end beyond the bytes":
            b2[-1] = len(data)
        elif what == "one byte beyond":
            b2[-1] += 1                                                   # (the last slice ends with the bytes)
        elif what == "negative begin":
            b2[0] = -1
        elif what == "n beyond the bytes":
            n2[-1] += 1
        else:
            n2[1] = 2 ** 31 - 1
        rc, bufs, _keep = _launch((data, b2, gt_type, n2, nal, amap), c.N)
        assert rc == _abi.VGL_E_ARG and b"GT slice" in lib.vgl_last_error(), what
        for buf, _ in bufs:                                               # no output byte was written: the decoder did not run
            assert bool((buf.cpu().numpy() == 0xA5).all()), what
    # a record without an integer type or without values has no slice: its gt_begin is not looked at
    t2, b2 = gt_type.copy(), begin.copy()
    t2[0], b2[0] = 5, -100
    rc, bufs, _keep = _launch((data, b2, t2, n, nal, amap), c.N)
    assert rc == _abi.VGL_OK
    status = bufs[2][1].cpu().numpy().view(np.int32)
    assert list(status) == [1, 0, 0, 0, 0]


def test_host_object_over_five_unequal_batches():
    """vgl_bcfin_host_*: two batches in flight, waited for in submit order; the results of a batch stay valid while the next one runs;
    the slices are picked out of the whole buffer (offsets relative to it)"""
    lib = _abi.load_library()
    c = bc.case_records(4097)
    data, begin, gt_type, n, nal, amap = c.arrays()
    rows, sums, status = c.expected()
    cuts = [0, 1, 1000, 1003, 3000, 4097]                                 # batches of 1, 999, 3, 1997 and 1097 records
    size = [c.slice_bytes(i) for i in range(len(begin))]
    max_gt = max(sum(size[a:b]) for a, b in zip(cuts, cuts[1:]))
    h = C.c_void_p()
    assert lib.vgl_bcfin_host_create(0, c.N, 2000, max_gt, C.byref(h)) == _abi.VGL_OK, lib.vgl_last_error()
    try:
        def submit(k, src=data, shift=0, records=None):
            a, b = (cuts[k], cuts[k + 1]) if records is None else records
            arrs = [np.ascontiguousarray(x) for x in (begin[a:b] + shift, gt_type[a:b], n[a:b], nal[a:b], amap[a:b])]
            ticket = C.c_int32(-1)
            rc = lib.vgl_bcfin_host_submit(h, src, len(src), b - a, *[x.ctypes.data for x in arrs], C.byref(ticket))
            return rc, ticket.value

        def wait(k, ticket):
            a, b = cuts[k], cuts[k + 1]
            g, s, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert lib.vgl_bcfin_host_wait(h, ticket, C.byref(g), C.byref(s), C.byref(st)) == _abi.VGL_OK, lib.vgl_last_error()
            got = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=((b - a) * c.N,)).reshape(b - a, c.N)
            got_s = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(b - a,))
            got_st = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_int32)), shape=(b - a,))
            return got, got_s, got_st

        tickets = []
        for k in range(5):
            rc, t = submit(k)                                             # batch k is enqueued before batch k - 1 is waited for
            assert rc == _abi.VGL_OK, lib.vgl_last_error()
            tickets.append(t)
            if k > 0:
                got, got_s, got_st = wait(k - 1, tickets[k - 1])
                a, b = cuts[k - 1], cuts[k]
                assert np.array_equal(got, rows[a:b]) and np.array_equal(got_s, sums[a:b]) and not got_st.any(), k
        got, got_s, got_st = wait(4, tickets[4])
        assert np.array_equal(got, rows[cuts[4]:]) and np.array_equal(got_s, sums[cuts[4]:]) and not got_st.any()
        # a ticket is waited for once; a third batch in flight, a slice outside the bytes and too many bytes or records are refused
        g = C.c_void_p()
        assert lib.vgl_bcfin_host_wait(h, tickets[4], C.byref(g), C.byref(g), C.byref(g)) == _abi.VGL_E_ARG
        (rc1, t1), (rc2, t2) = submit(0), submit(1)
        assert rc1 == rc2 == _abi.VGL_OK
        assert submit(2)[0] == _abi.VGL_E_ARG and b"in flight" in lib.vgl_last_error()
        assert np.array_equal(wait(0, t1)[0], rows[:1]) and np.array_equal(wait(1, t2)[0], rows[1:1000])
        last = (4096, 4097)
        assert submit(0, src=data[:-1], records=last)[0] == _abi.VGL_E_ARG and b"GT slice" in lib.vgl_last_error()
        assert submit(0, shift=1, records=last)[0] == _abi.VGL_E_ARG
        assert submit(0, shift=-int(begin[4096]) - 1, records=last)[0] == _abi.VGL_E_ARG
        assert submit(0, records=(0, 2001))[0] == _abi.VGL_E_ARG
        assert submit(0, records=(1000, 3000))[0] == _abi.VGL_E_ARG and b"max_gt_bytes" in lib.vgl_last_error()
        rc, t = submit(0, records=last)                                   # the handle is still good
        assert rc == _abi.VGL_OK
        g, s, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.vgl_bcfin_host_wait(h, t, C.byref(g), C.byref(s), C.byref(st)) == _abi.VGL_OK
        assert bytes(np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=(c.N,))) == bytes(rows[4096])
    finally:
        assert lib.vgl_bcfin_host_destroy(h) == _abi.VGL_OK
