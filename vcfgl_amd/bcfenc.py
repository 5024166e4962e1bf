"""The FORMAT part of BCF records on the device (libvcfgl_hip.so, ABI 7: vgl_bcf_encode_device).

For every kept site of a tile (site_status >= 0) the bytes are the `indiv` block the host writer puts behind a record's shared block:
per field the typed dictionary id of its key, the size/type byte and the values of all samples in the narrowest integer type that
holds the record's range (float32 fields as bit patterns) -- encoded from the tile's sample-major FORMAT slabs
(VGL_LAYOUT_SAMPLE_MAJOR) where they are computed, byte for byte as the host program encodes them.  Skipped sites have no bytes.

    fields = bcfenc.tile_fields(args, tile, key_ids)          # key_ids: {"DP": 3, "GL": 4, ...} from the output header's dictionary
    data, offsets = bcfenc.encode_records(fields, tile["site_status"], tile["n_alleles"], n_samples)
    # site i's FORMAT bytes: data[offsets[i]:offsets[i + 1]]
"""
import ctypes as C

from . import _abi
from .vcftext import FORMAT_ORDER

ONE, PER_G, PER_A = _abi.VGL_TEXT_ONE, _abi.VGL_TEXT_PER_G, _abi.VGL_TEXT_PER_A
# the order of vgl_ctx_bcf_keys' seven dictionary ids
KEY_ORDER = [key for key, _, _, _, _ in FORMAT_ORDER]


def tile_fields(args, tile, key_ids):
    """[(key id, tensor, kind)] of the tags `args` enables, from a device Tile (or a dict of [n_sites, ...] tensors)"""
    return [(int(key_ids[key]), tile[name], kind) for key, name, _, kind, flag in FORMAT_ORDER if getattr(args, flag)]


def _descriptors(fields, n_sites):
    import torch
    arr = (_abi.BcfField * max(1, len(fields)))()
    for k, (key_id, t, kind) in enumerate(fields):
        if t.dtype not in (torch.float32, torch.int32) or not t.is_contiguous() or t.shape[0] != n_sites:
            raise ValueError(f"bcfenc: field {k} (key id {key_id}): a contiguous float32 / int32 tensor [n_sites, ...] is expected")
        arr[k] = _abi.BcfField(int(key_id), 1 if t.dtype == torch.float32 else 0, kind, t.data_ptr(), t[0].numel() if n_sites else 0)
    return arr


def bound(fields, n_sites, n_samples, max_alleles=5):
    """largest encoding of n_sites sites (host arithmetic)"""
    arr = (_abi.BcfField * max(1, len(fields)))()
    for k, (key_id, t, kind) in enumerate(fields):
        arr[k] = _abi.BcfField(int(key_id), 1 if str(t.dtype).endswith("float32") else 0, kind, None, 0)
    return int(_abi.load_library().vgl_bcf_bound(n_samples, n_sites, arr, len(fields), max_alleles))


def encode_into(fields, site_status, n_alleles, n_samples, dst, dst_cap=None):
    """encode into the device uint8 tensor `dst` (at most dst_cap bytes) on the current stream; returns the device offsets
    [n_sites + 1] without waiting.  When offsets[n_sites] > dst_cap nothing was written."""
    import torch
    n_sites = int(site_status.shape[0])
    dev = site_status.device
    lib = _abi.load_library()
    arr = _descriptors(fields, n_sites)
    cap = dst.numel() if dst_cap is None else int(dst_cap)
    if cap > dst.numel():
        raise ValueError("bcfenc.encode_into: dst_cap exceeds dst")
    with torch.cuda.device(dev):
        offsets = torch.empty(n_sites + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(lib.vgl_bcf_workspace_bytes(n_samples, n_sites))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_bcf_encode_device(dev.index, arr, len(fields), n_samples, n_sites, C.c_void_p(site_status.data_ptr()),
                                       C.c_void_p(n_alleles.data_ptr()), C.c_void_p(dst.data_ptr()), cap, C.c_void_p(offsets.data_ptr()),
                                       C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != _abi.VGL_OK:
            raise RuntimeError(f"vgl_bcf_encode_device: {lib.vgl_last_error().decode()} (code {rc})")
        ws.record_stream(stream)
        return offsets


def encode_records(fields, site_status, n_alleles, n_samples):
    """(data, offsets): the FORMAT bytes of every kept site as one device uint8 tensor and the int64 site offsets [n_sites + 1]
    (both on the device of site_status).  fields = [(key id, tensor [n_sites, ...] sample-major, ONE / PER_G / PER_A)].  Waits for
    the current stream (the size comes back)."""
    import torch
    for t in (site_status, n_alleles):
        if t.dtype != torch.int32 or t.device.type != "cuda":
            raise ValueError("bcfenc.encode_records: int32 site_status / n_alleles on a HIP device are expected")
    n_sites = int(site_status.shape[0])
    dst = torch.empty(max(1, bound(fields, n_sites, n_samples)), dtype=torch.uint8, device=site_status.device)
    offsets = encode_into(fields, site_status, n_alleles, n_samples, dst)
    total = int(offsets[-1].item())
    return dst[:total].clone(), offsets
