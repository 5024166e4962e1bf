"""Pileup lines on the device (libvcfgl_hip.so, ABI 7: vgl_pileup_format_device).

For every site of a tile that is not VGL_SITE_SKIP_EMPTY the text is what the host writer appends behind a -printPileup 1 line's
prefix (chrom, pos, ref): one "\\t" column per sample, "0\\t*\\t*" for a sample without reads, else dp "\\t" bases "\\t" scores, then
"\\n".  It is formatted from the tile's DP plane and read dump where they are computed, byte for byte as the host program writes it.

    text, offsets = pileup.format_columns(tile["site_status"], tile["fmt_dp"], reads, n_samples)
    # site i's text: text[offsets[i]:offsets[i + 1]]; reads: uint8 [read_capacity, n_sites, n_samples] (vgl_tile_out.reads)
"""
import ctypes as C

from . import _abi


def bound(n_samples, n_sites, read_capacity):
    """largest text of n_sites sites whose depths are at most read_capacity (host arithmetic)"""
    return int(_abi.load_library().vgl_pileup_bound(n_samples, n_sites, read_capacity))


def format_into(site_status, fmt_dp, reads, n_samples, dst, dst_cap=None, qual_char=-1):
    """format into the device uint8 tensor `dst` (at most dst_cap bytes) on the current stream; returns the device offsets
    [n_sites + 1] without waiting.  When offsets[n_sites] > dst_cap nothing was written; offsets[n_sites] = -1: a depth out of
    [0, read_capacity], nothing was written."""
    import torch
    n_sites = int(site_status.shape[0])
    dev = site_status.device
    read_capacity = int(reads.shape[0])
    if reads.dtype != torch.uint8 or not reads.is_contiguous() or tuple(reads.shape[1:]) != (n_sites, n_samples):
        raise ValueError("pileup: reads must be a contiguous uint8 tensor [read_capacity, n_sites, n_samples]")
    if fmt_dp.dtype != torch.int32 or not fmt_dp.is_contiguous() or fmt_dp.numel() != n_sites * n_samples:
        raise ValueError("pileup: fmt_dp must be a contiguous int32 tensor [n_sites, n_samples]")
    lib = _abi.load_library()
    cap = dst.numel() if dst_cap is None else int(dst_cap)
    if cap > dst.numel():
        raise ValueError("pileup.format_into: dst_cap exceeds dst")
    with torch.cuda.device(dev):
        offsets = torch.empty(n_sites + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(lib.vgl_pileup_workspace_bytes(n_samples, n_sites))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_pileup_format_device(dev.index, n_samples, n_sites, C.c_void_p(site_status.data_ptr()), C.c_void_p(fmt_dp.data_ptr()),
                                          C.c_void_p(reads.data_ptr()), read_capacity, int(qual_char), C.c_void_p(dst.data_ptr()), cap,
                                          C.c_void_p(offsets.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != _abi.VGL_OK:
            raise RuntimeError(f"vgl_pileup_format_device: {lib.vgl_last_error().decode()} (code {rc})")
        ws.record_stream(stream)
        return offsets


def format_columns(site_status, fmt_dp, reads, n_samples, qual_char=-1):
    """(text, offsets): the pileup columns of every site but the empty ones as one device uint8 tensor and the int64 site offsets
    [n_sites + 1] (both on the device of site_status).  reads: uint8 [read_capacity, n_sites, n_samples]; qual_char = -1: each
    read's own score + 33, else this byte for every read.  Waits for the current stream (the size of the text comes back); a depth
    out of [0, read_capacity] raises ValueError."""
    import torch
    if site_status.dtype != torch.int32 or site_status.device.type != "cuda":
        raise ValueError("pileup.format_columns: int32 site_status on a HIP device is expected")
    n_sites = int(site_status.shape[0])
    dst = torch.empty(max(1, bound(n_samples, n_sites, int(reads.shape[0]))), dtype=torch.uint8, device=site_status.device)
    offsets = format_into(site_status, fmt_dp, reads, n_samples, dst, qual_char=qual_char)
    total = int(offsets[-1].item())
    if total < 0:
        raise ValueError("pileup.format_columns: a depth is negative or exceeds the read dump's capacity")
    return dst[:total].clone(), offsets
