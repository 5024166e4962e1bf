"""A tile's record stream assembled and compressed on the device (libvcfgl_hip.so, ABI 7: vgl_stream_assemble_device,
vgl_stream_host_*).

A record is a head the host builds (the eight fixed columns of a VCF line; l_shared, l_indiv and the shared block of a BCF record)
followed by the body the device built (vcftext / bcfenc).  `assemble` interleaves the two on the device, site by site:

    data, total = stream.assemble(heads, head_offsets, bodies, body_offsets)      # device tensors; record i starts at
    # (head_offsets[i] - head_offsets[0]) + (body_offsets[i] - body_offsets[0])

`HostStream` is the handle a record loop uses: the tile call writes its bodies into `body(k)`, `submit` sends the heads up and
enqueues assembly and BGZF compression, `wait` returns the members (without the EOF member).
"""
import ctypes as C

from . import _abi


def _check(lib, rc, what):
    if rc != _abi.VGL_OK:
        raise RuntimeError(f"{what}: {lib.vgl_last_error().decode()} (code {rc})")


def assemble_into(heads, head_offsets, bodies, body_offsets, dst, dst_cap=None):
    """assemble into the device uint8 tensor `dst` (at most dst_cap bytes) on the current stream; returns the device int64 tensor [1]
    that receives the stream's length, without waiting.  When it exceeds dst_cap nothing was written."""
    import torch
    for t in (head_offsets, body_offsets):
        if t.dtype != torch.int64 or t.device.type != "cuda" or not t.is_contiguous():
            raise ValueError("stream.assemble_into: contiguous int64 offsets on a HIP device are expected")
    for t in (heads, bodies, dst):
        if t.dtype != torch.uint8 or t.device.type != "cuda" or not t.is_contiguous():
            raise ValueError("stream.assemble_into: contiguous uint8 tensors on a HIP device are expected")
    if head_offsets.numel() != body_offsets.numel() or head_offsets.numel() < 1:
        raise ValueError("stream.assemble_into: both offset arrays hold n_sites + 1 entries")
    n_sites = head_offsets.numel() - 1
    dev = dst.device
    cap = dst.numel() if dst_cap is None else int(dst_cap)
    if cap > dst.numel():
        raise ValueError("stream.assemble_into: dst_cap exceeds dst")
    lib = _abi.load_library()
    with torch.cuda.device(dev):
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_stream_assemble_device(dev.index, n_sites, C.c_void_p(heads.data_ptr()), C.c_void_p(head_offsets.data_ptr()),
                                            C.c_void_p(bodies.data_ptr()), C.c_void_p(body_offsets.data_ptr()), C.c_void_p(dst.data_ptr()),
                                            cap, C.c_void_p(total.data_ptr()), C.c_void_p(stream.cuda_stream))
        _check(lib, rc, "vgl_stream_assemble_device")
        return total


def assemble(heads, head_offsets, bodies, body_offsets):
    """(data, total): the records of the tile as one device uint8 tensor and its length.  Waits for the current stream (the offsets'
    totals size the result)."""
    import torch
    n = int((head_offsets[-1] - head_offsets[0] + body_offsets[-1] - body_offsets[0]).item())
    dst = torch.empty(max(1, n), dtype=torch.uint8, device=heads.device)
    total = int(assemble_into(heads, head_offsets, bodies, body_offsets, dst, dst_cap=n).item())
    return dst[:total], total


class HostStream:
    """vgl_stream_host_*: n_buffers device body buffers, one stream of assembly + compression, members back in page-locked memory"""

    def __init__(self, device, n_buffers, max_sites, max_head_bytes, max_body_bytes):
        self.lib = _abi.load_library()
        self.h = C.c_void_p()
        self.n_buffers, self.max_body_bytes = n_buffers, max_body_bytes
        _check(self.lib, self.lib.vgl_stream_host_create(device, n_buffers, max_sites, max_head_bytes, max_body_bytes, C.byref(self.h)),
               "vgl_stream_host_create")

    def body(self, k):
        """device address of body buffer k (the `text` of a tile call on a context with vgl_ctx_text_device)"""
        p = self.lib.vgl_stream_host_body(self.h, k)
        if not p:
            raise RuntimeError(f"vgl_stream_host_body: {self.lib.vgl_last_error().decode()}")
        return p

    def submit_rc(self, k, heads, head_offsets, body_offsets):
        """(return code, ticket) of vgl_stream_host_submit on numpy arrays (uint8 heads, int64 offsets [n_sites + 1])"""
        t = C.c_int32(-1)
        n_sites = len(head_offsets) - 1
        rc = self.lib.vgl_stream_host_submit(self.h, k, n_sites, heads.ctypes.data, head_offsets.ctypes.data, body_offsets.ctypes.data, C.byref(t))
        return rc, t.value

    def submit(self, k, heads, head_offsets, body_offsets):
        rc, t = self.submit_rc(k, heads, head_offsets, body_offsets)
        _check(self.lib, rc, "vgl_stream_host_submit")
        return t

    def wait(self, ticket):
        """(members, raw_n): the ticket's BGZF members as bytes (without the EOF member) and the length they decompress to"""
        p, n, raw = C.c_void_p(), C.c_int64(), C.c_int64()
        _check(self.lib, self.lib.vgl_stream_host_wait(self.h, ticket, C.byref(p), C.byref(n), C.byref(raw)), "vgl_stream_host_wait")
        return (C.string_at(p.value, n.value) if n.value else b""), raw.value

    def close(self):
        if self.h:
            self.lib.vgl_stream_host_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
