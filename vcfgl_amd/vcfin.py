"""The sample columns of VCF text parsed on the device (vgl_vcfin.hip; include/vcfgl_hip.h, "the sample columns of VCF text").

`parse_gt` takes device tensors: the text as uint8, per line the offsets of its sample region, the index of GT in FORMAT, the
allele count and the five-entry map from allele index to the nibble the tile calls take.  It returns the packed rows
[n_lines][n_samples], the allele sums and the statuses: a line with status VCFIN_HOST is outside the plain grammar and is
left to the caller's own parser (its row is unspecified).
"""
import ctypes as C

from . import _abi

VCFIN_OK, VCFIN_HOST = _abi.VCFIN_OK, _abi.VCFIN_HOST


def parse_gt(text, line_begin, line_end, gti, n_alleles, allele_map, n_samples, device=None, stream=None, lib=None):
    """text uint8 [text_bytes]; line_begin, line_end int64 [n_lines]; gti, n_alleles int32 [n_lines]; allele_map int8 [n_lines][5];
    all contiguous tensors on one device (`device`: a torch device or ordinal; the text's device when None).
    Returns (gt uint8 [n_lines][n_samples], allelesum int32 [n_lines], status int32 [n_lines]) on that device.  The line ranges
    are checked against the text by a small kernel whose one word the call waits for on `stream` (ValueError for a range outside
    the text; the parser is then not launched); the parse itself is enqueued on `stream` and not waited for.  `stream` is a HIP
    stream handle; None takes torch's current stream of the device."""
    import torch
    lib = lib or _abi.load_library()
    dev = text.device if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("parse_gt takes device tensors")
    n_lines = int(line_begin.numel())
    want = ((text, torch.uint8, text.numel()), (line_begin, torch.int64, n_lines), (line_end, torch.int64, n_lines),
            (gti, torch.int32, n_lines), (n_alleles, torch.int32, n_lines), (allele_map, torch.int8, 5 * n_lines))
    for t, dt, n in want:
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != text.device:
            raise ValueError("parse_gt: text uint8, line_begin / line_end int64 [n_lines], gti / n_alleles int32 [n_lines], "
                             "allele_map int8 [n_lines][5], contiguous and on one device")
    if text.device.index != (dev.index or 0) and dev.index is not None:
        raise ValueError("parse_gt: the tensors are not on the device asked for")
    gt = torch.empty((n_lines, n_samples), dtype=torch.uint8, device=text.device)
    allelesum = torch.empty(n_lines, dtype=torch.int32, device=text.device)
    status = torch.empty(n_lines, dtype=torch.int32, device=text.device)
    ws = torch.empty(max(int(lib.vgl_vcfin_workspace_bytes(n_samples, n_lines)), 1), dtype=torch.uint8, device=text.device)
    rc = lib.vgl_vcfin_parse_device(text.device.index or 0, text.data_ptr(), text.numel(), n_lines, line_begin.data_ptr(), line_end.data_ptr(),
                                    gti.data_ptr(), n_alleles.data_ptr(), allele_map.data_ptr(), n_samples, gt.data_ptr(),
                                    allelesum.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                    C.c_void_p(stream if stream else torch.cuda.current_stream(text.device).cuda_stream))
    if rc == _abi.VGL_E_ARG:
        raise ValueError("vgl_vcfin_parse_device: %s" % lib.vgl_last_error().decode())
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_vcfin_parse_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return gt, allelesum, status
