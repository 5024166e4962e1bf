"""VCF text of the sample columns on the device (libvcfgl_hip.so, ABI 7: vgl_text_format_device).

For every kept site of a tile (site_status >= 0) the text is what the host writer appends behind a record's eight fixed columns --
"\\t" KEYS, one "\\t" column per sample, "\\n" -- formatted from the tile's sample-major FORMAT slabs (VGL_LAYOUT_SAMPLE_MAJOR) where
they are computed, byte for byte as the host program formats them.  Skipped sites have no text.

    fields = vcftext.tile_fields(args, tile)                  # the tags args enables, in add_tags() order, from a device Tile
    text, offsets = vcftext.format_columns(fields, tile["site_status"], tile["n_alleles"], n_samples)
    # site i's text: text[offsets[i]:offsets[i + 1]]
"""
import ctypes as C

from . import _abi

ONE, PER_G, PER_A = _abi.VGL_TEXT_ONE, _abi.VGL_TEXT_PER_G, _abi.VGL_TEXT_PER_A
# the FORMAT tags of a simulated record in add_tags() order: (key, tile field, float?, count kind, the VcfglArgs flag)
FORMAT_ORDER = [("DP", "fmt_dp", False, ONE, "add_fmt_dp"), ("GL", "gl", True, PER_G, "add_gl"), ("PL", "pl", False, PER_G, "add_pl"),
                ("GP", "gp", True, PER_G, "add_gp"), ("AD", "fmt_ad", False, PER_A, "add_fmt_ad"),
                ("ADF", "fmt_adf", False, PER_A, "add_fmt_adf"), ("ADR", "fmt_adr", False, PER_A, "add_fmt_adr")]


def tile_fields(args, tile):
    """[(key, tensor, kind)] of the tags `args` enables, from a device Tile (or a dict of [n_sites, ...] tensors)"""
    return [(key, tile[name], kind) for key, name, _, kind, flag in FORMAT_ORDER if getattr(args, flag)]


def _descriptors(fields, n_sites):
    import torch
    arr = (_abi.TextField * max(1, len(fields)))()
    keep = []
    for k, (key, t, kind) in enumerate(fields):
        if t.dtype not in (torch.float32, torch.int32) or not t.is_contiguous() or t.shape[0] != n_sites:
            raise ValueError(f"vcftext: field {key}: a contiguous float32 / int32 tensor [n_sites, ...] is expected")
        kb = key.encode()
        keep.append(kb)
        arr[k] = _abi.TextField(kb, 1 if t.dtype == torch.float32 else 0, kind, t.data_ptr(), t[0].numel() if n_sites else 0)
    return arr, keep


def bound(fields, n_sites, n_samples, max_alleles=5):
    """largest text of n_sites sites (host arithmetic)"""
    arr = (_abi.TextField * max(1, len(fields)))()
    for k, (key, t, kind) in enumerate(fields):
        arr[k] = _abi.TextField(key.encode(), 1 if str(t.dtype).endswith("float32") else 0, kind, None, 0)
    return int(_abi.load_library().vgl_text_bound(n_samples, n_sites, arr, len(fields), max_alleles))


def format_into(fields, site_status, n_alleles, n_samples, dst, dst_cap=None):
    """format into the device uint8 tensor `dst` (at most dst_cap bytes) on the current stream; returns the device offsets
    [n_sites + 1] without waiting.  When offsets[n_sites] > dst_cap nothing was written."""
    import torch
    n_sites = int(site_status.shape[0])
    dev = site_status.device
    lib = _abi.load_library()
    arr, keep = _descriptors(fields, n_sites)
    cap = dst.numel() if dst_cap is None else int(dst_cap)
    if cap > dst.numel():
        raise ValueError("vcftext.format_into: dst_cap exceeds dst")
    with torch.cuda.device(dev):
        offsets = torch.empty(n_sites + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(lib.vgl_text_workspace_bytes(n_samples, n_sites))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_text_format_device(dev.index, arr, len(fields), n_samples, n_sites, C.c_void_p(site_status.data_ptr()),
                                        C.c_void_p(n_alleles.data_ptr()), C.c_void_p(dst.data_ptr()), cap, C.c_void_p(offsets.data_ptr()),
                                        C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != _abi.VGL_OK:
            raise RuntimeError(f"vgl_text_format_device: {lib.vgl_last_error().decode()} (code {rc})")
        ws.record_stream(stream)
        del keep
        return offsets


def format_columns(fields, site_status, n_alleles, n_samples):
    """(text, offsets): the sample columns of every kept site as one device uint8 tensor and the int64 site offsets [n_sites + 1]
    (both on the device of site_status).  fields = [(key, tensor [n_sites, ...] sample-major, ONE / PER_G / PER_A)].  Waits for the
    current stream (the size of the text comes back)."""
    import torch
    for t in (site_status, n_alleles):
        if t.dtype != torch.int32 or t.device.type != "cuda":
            raise ValueError("vcftext.format_columns: int32 site_status / n_alleles on a HIP device are expected")
    n_sites = int(site_status.shape[0])
    dst = torch.empty(max(1, bound(fields, n_sites, n_samples)), dtype=torch.uint8, device=site_status.device)
    offsets = format_into(fields, site_status, n_alleles, n_samples, dst)
    total = int(offsets[-1].item())
    return dst[:total].clone(), offsets
