"""The FORMAT/GT vectors of BCF records decoded on the device (vgl_bcfin.hip; include/vcfgl_hip.h, "the FORMAT/GT vectors of BCF
records").

`decode_gt` takes device tensors: the bytes that hold the records' GT slices as uint8, per record the offset of its slice, the BCF
type of its values (1 int8, 2 int16, 3 int32), the number of values per sample, the allele count and the five-entry map from allele
index to the nibble the tile calls take.  It returns the packed rows [n_records][n_samples], the allele sums and the statuses: a
record with status BCFIN_HOST is outside the plain rule and is left to the caller's own decoder (its row is unspecified).
"""
import ctypes as C

from . import _abi

BCFIN_OK, BCFIN_HOST = _abi.BCFIN_OK, _abi.BCFIN_HOST


def decode_gt(gt_bytes, gt_begin, gt_type, gt_n, n_alleles, allele_map, n_samples, device=None, stream=None, lib=None):
    """gt_bytes uint8 [bytes]; gt_begin int64 [n_records]; gt_type, gt_n, n_alleles int32 [n_records]; allele_map int8 [n_records][5];
    all contiguous tensors on one device (`device`: a torch device or ordinal; the bytes' device when None).
    Returns (gt uint8 [n_records][n_samples], allelesum int32 [n_records], status int32 [n_records]) on that device.  The slices are
    checked against the bytes by a small kernel whose one word the call waits for on `stream` (ValueError for a slice outside the
    bytes; the decoder is then not launched); the decode itself is enqueued on `stream` and not waited for.  `stream` is a HIP
    stream handle; None takes torch's current stream of the device."""
    import torch
    lib = lib or _abi.load_library()
    dev = gt_bytes.device if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("decode_gt takes device tensors")
    n_records = int(gt_begin.numel())
    want = ((gt_bytes, torch.uint8, gt_bytes.numel()), (gt_begin, torch.int64, n_records), (gt_type, torch.int32, n_records),
            (gt_n, torch.int32, n_records), (n_alleles, torch.int32, n_records), (allele_map, torch.int8, 5 * n_records))
    for t, dt, n in want:
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != gt_bytes.device:
            raise ValueError("decode_gt: gt_bytes uint8, gt_begin int64 [n_records], gt_type / gt_n / n_alleles int32 [n_records], "
                             "allele_map int8 [n_records][5], contiguous and on one device")
    if gt_bytes.device.index != (dev.index or 0) and dev.index is not None:
        raise ValueError("decode_gt: the tensors are not on the device asked for")
    gt = torch.empty((n_records, n_samples), dtype=torch.uint8, device=gt_bytes.device)
    allelesum = torch.empty(n_records, dtype=torch.int32, device=gt_bytes.device)
    status = torch.empty(n_records, dtype=torch.int32, device=gt_bytes.device)
    ws = torch.empty(max(int(lib.vgl_bcfin_workspace_bytes(n_samples, n_records)), 1), dtype=torch.uint8, device=gt_bytes.device)
    rc = lib.vgl_bcfin_decode_device(gt_bytes.device.index or 0, gt_bytes.data_ptr(), gt_bytes.numel(), n_records, gt_begin.data_ptr(),
                                     gt_type.data_ptr(), gt_n.data_ptr(), n_alleles.data_ptr(), allele_map.data_ptr(), n_samples,
                                     gt.data_ptr(), allelesum.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                     C.c_void_p(stream if stream else torch.cuda.current_stream(gt_bytes.device).cuda_stream))
    if rc == _abi.VGL_E_ARG:
        raise ValueError("vgl_bcfin_decode_device: %s" % lib.vgl_last_error().decode())
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_bcfin_decode_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return gt, allelesum, status
