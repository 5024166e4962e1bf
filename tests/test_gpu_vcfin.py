"""k_vcfin_parse (vgl_vcfin.hip) against tests/vcfin_model.py, exact equality: the line sets of tests/vcfin_cases.py (sample counts,
line counts, region lengths around the chunk and lane sizes, every alignment, GT as subfield 0 .. 2, every kind of line outside
the plain grammar), guard bands around the three outputs, the argument checks, the Python wrapper and the host object."""
import ctypes as C

import numpy as np
import pytest
import torch

import vcfin_cases as vc
import vcfin_model as vm
from vcfgl_amd import _abi, vcfin

pytestmark = pytest.mark.gpu
GUARD = 64


def _guarded(n_bytes, dev):
    """a device buffer of n_bytes between two guard bands of 0xA5 (the payload starts on a 64-byte boundary)"""
    buf = torch.full((GUARD + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n_bytes]


def _intact(buf, n_bytes):
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == 0xA5).all() and (h[GUARD + n_bytes:] == 0xA5).all())


def run_device(case, text_shift=0):
    """the entry point on a case, outputs between guard bands; text_shift moves the text against the allocation's alignment"""
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    text, lb, le, gti, nal, amap = case.arrays()
    n, N = len(lb), case.N
    t_all = torch.zeros(text_shift + len(text), dtype=torch.uint8, device=dev)
    t_all[text_shift:] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_text = t_all[text_shift:]
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (lb, le, gti, nal, amap)]
    g_buf, g = _guarded(n * N, dev)
    s_buf, s = _guarded(n * 4, dev)
    st_buf, st = _guarded(n * 4, dev)
    ws = torch.zeros(int(lib.vgl_vcfin_workspace_bytes(N, n)), dtype=torch.uint8, device=dev)
    rc = lib.vgl_vcfin_parse_device(0, d_text.data_ptr(), len(text), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                    d[4].data_ptr(), N, g.data_ptr(), s.data_ptr(), st.data_ptr(), ws.data_ptr(), None)
    assert rc == _abi.VGL_OK, lib.vgl_last_error()
    torch.cuda.synchronize()
    assert _intact(g_buf, n * N) and _intact(s_buf, n * 4) and _intact(st_buf, n * 4)
    return (g.cpu().numpy().reshape(n, N), s.cpu().numpy().view(np.int32), st.cpu().numpy().view(np.int32))


def check(case, **kw):
    rows, sums, status = case.expected()
    got_rows, got_sums, got_status = run_device(case, **kw)
    assert np.array_equal(got_status, status)
    ok = status == vm.VCFIN_OK
    assert {int(i) for i in np.nonzero(~ok)[0]} == case.fallback          # exactly the constructed lines are handed back
    assert np.array_equal(got_sums[ok], sums[ok])
    assert np.array_equal(got_rows[ok], rows[ok])
    return got_rows, got_sums, got_status


@pytest.mark.parametrize("n", vc.SAMPLE_COUNTS)
def test_sample_counts(n):
    check(vc.case_samples(n))


@pytest.mark.parametrize("n_lines", vc.LINE_COUNTS)
def test_line_counts(n_lines):
    check(vc.case_lines(n_lines))


@pytest.mark.parametrize("length", vc.REGION_LENGTHS)
def test_region_lengths_around_the_lane_and_chunk_sizes(length):
    check(vc.case_region(length))


def test_tokens_straddle_every_lane_and_chunk_boundary_at_every_alignment():
    c = vc.case_straddle()
    rows, _, _ = check(c)
    assert all(np.array_equal(rows[0], r) for r in rows)                  # the same columns on all 17 lines
    check(c, text_shift=5)                                                # and with the text itself off the 16-byte boundaries


def test_gt_as_subfield_0_1_2():
    check(vc.case_gti())


def test_lines_outside_the_grammar_are_handed_back_and_their_neighbours_are_intact():
    c = vc.case_fallback()
    rows, sums, status = check(c)                                         # (guard bands: a line with N + 3 columns writes N bytes)
    assert status.sum() == len(vc.FALLBACK_KINDS) and status[0] == status[-1] == vm.VCFIN_OK


def test_lines_the_five_entry_map_cannot_describe_are_handed_back():
    """n_alleles outside 1 .. 5 and a negative gti through the C ABI: the caller's lines, whatever their tokens"""
    c = vc.Case(66)
    cols = [b"0|1"] * 66
    c.add(cols).add(cols, nal=6, fallback=True).add(cols, nal=0, fallback=True).add(cols, gti=-1, fallback=True).add(cols, nal=5)
    rows, sums, status = check(c)
    assert list(status) == [0, 1, 1, 1, 0] and np.array_equal(rows[0], rows[4])


def test_python_wrapper():
    c = vc.case_samples(257)
    text, lb, le, gti, nal, amap = c.arrays()
    dev = torch.device("cuda", 0)
    t = [torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)] + [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (lb, le, gti, nal, amap)]
    gt, sums, status = vcfin.parse_gt(*t, c.N, device=0)
    rows, want_sums, want_status = c.expected()
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (len(lb), c.N) and sums.dtype == status.dtype == torch.int32
    assert np.array_equal(gt.cpu().numpy(), rows) and np.array_equal(sums.cpu().numpy(), want_sums) and not status.cpu().numpy().any()
    with pytest.raises(ValueError):
        vcfin.parse_gt(t[0], t[1].to(torch.int32), *t[2:], c.N)


def test_line_ranges_outside_the_text_are_refused_and_nothing_is_launched():
    lib = _abi.load_library()
    c = vc.case_samples(64)
    text, lb, le, gti, nal, amap = c.arrays()
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    for what in ("end beyond the text", "begin behind end", "negative begin"):
        lb2, le2 = lb.copy(), le.copy()
        if what == "end beyond the text":
            le2[-1] = len(text) + 1
        elif what == "begin behind end":
            lb2[1] = le2[1] + 1
        else:
            lb2[0] = -1
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (lb2, le2, gti, nal, amap)]
        n, N = len(lb), c.N
        g_buf, g = _guarded(n * N, dev)
        s_buf, s = _guarded(n * 4, dev)
        st_buf, st = _guarded(n * 4, dev)
        ws = torch.zeros(int(lib.vgl_vcfin_workspace_bytes(N, n)), dtype=torch.uint8, device=dev)
        rc = lib.vgl_vcfin_parse_device(0, d_text.data_ptr(), len(text), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                        d[4].data_ptr(), N, g.data_ptr(), s.data_ptr(), st.data_ptr(), ws.data_ptr(), None)
        assert rc == _abi.VGL_E_ARG and b"line range" in lib.vgl_last_error(), what
        torch.cuda.synchronize()
        for buf in (g_buf, s_buf, st_buf):                                # no output byte was written: the parser did not run
            assert bool((buf.cpu().numpy() == 0xA5).all()), what
    with pytest.raises(ValueError):
        le2 = le.copy(); le2[0] = len(text) + 100
        vcfin.parse_gt(d_text, *[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (lb, le2, gti, nal, amap)], c.N)


def test_host_object_over_five_unequal_batches():
    """vgl_vcfin_host_*: two batches in flight, waited for in submit order; the results of a batch stay valid while the next one runs"""
    lib = _abi.load_library()
    c = vc.case_lines(4097)
    text, lb, le, gti, nal, amap = c.arrays()
    rows, sums, status = c.expected()
    cuts = [0, 1, 1000, 1003, 3000, 4097]                                 # batches of 1, 999, 3, 1997 and 1097 lines
    h = C.c_void_p()
    max_text = max(int(le[b - 1] - lb[a]) for a, b in zip(cuts, cuts[1:]))
    assert lib.vgl_vcfin_host_create(0, c.N, 2000, max_text, C.byref(h)) == _abi.VGL_OK, lib.vgl_last_error()
    try:
        def submit(k):
            a, b = cuts[k], cuts[k + 1]
            t0 = int(lb[a])
            sub = text[t0:int(le[b - 1])]
            arrs = [np.ascontiguousarray(x) for x in (lb[a:b] - t0, le[a:b] - t0, gti[a:b], nal[a:b], amap[a:b])]
            ticket = C.c_int32(-1)
            rc = lib.vgl_vcfin_host_submit(h, sub, len(sub), b - a, *[x.ctypes.data for x in arrs], C.byref(ticket))
            assert rc == _abi.VGL_OK, lib.vgl_last_error()
            return ticket.value

        def wait(k, ticket):
            a, b = cuts[k], cuts[k + 1]
            g, s, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert lib.vgl_vcfin_host_wait(h, ticket, C.byref(g), C.byref(s), C.byref(st)) == _abi.VGL_OK, lib.vgl_last_error()
            got = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=((b - a) * c.N,)).reshape(b - a, c.N)
            got_s = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(b - a,))
            got_st = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_int32)), shape=(b - a,))
            return got, got_s, got_st

        tickets = [submit(0)]
        for k in range(1, 5):
            tickets.append(submit(k))                                     # batch k is enqueued before batch k - 1 is waited for
            got, got_s, got_st = wait(k - 1, tickets[k - 1])
            a, b = cuts[k - 1], cuts[k]
            assert np.array_equal(got, rows[a:b]) and np.array_equal(got_s, sums[a:b]) and not got_st.any(), k
        third = C.c_int32(-1)
        got, got_s, got_st = wait(4, tickets[4])
        assert np.array_equal(got, rows[cuts[4]:]) and np.array_equal(got_s, sums[cuts[4]:]) and not got_st.any()
        # a ticket is waited for once; a third batch in flight and a range outside the text are refused
        g = C.c_void_p()
        assert lib.vgl_vcfin_host_wait(h, tickets[4], C.byref(g), C.byref(g), C.byref(g)) == _abi.VGL_E_ARG
        t1, t2 = submit(0), submit(1)
        one = [np.ascontiguousarray(x) for x in (lb[:1] - lb[0], le[:1] - lb[0], gti[:1], nal[:1], amap[:1])]
        sub = text[int(lb[0]):int(le[0])]
        assert lib.vgl_vcfin_host_submit(h, sub, len(sub), 1, *[x.ctypes.data for x in one], C.byref(third)) == _abi.VGL_E_ARG
        assert np.array_equal(wait(0, t1)[0], rows[:1]) and np.array_equal(wait(1, t2)[0], rows[1:1000])
        bad = one[1] + 1
        assert lib.vgl_vcfin_host_submit(h, sub, len(sub), 1, one[0].ctypes.data, bad.ctypes.data, *[x.ctypes.data for x in one[2:]],
                                         C.byref(third)) == _abi.VGL_E_ARG
        assert lib.vgl_vcfin_host_submit(h, sub, len(sub), 2001, *[x.ctypes.data for x in one], C.byref(third)) == _abi.VGL_E_ARG
    finally:
        assert lib.vgl_vcfin_host_destroy(h) == _abi.VGL_OK
