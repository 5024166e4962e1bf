"""One genotype's FORMAT/GL of every sample as CSV text, formatted on the device (vgl_fetchgl.hip; include/vcfgl_hip.h, "one
genotype's FORMAT/GL as CSV text"): what the reference's misc/fetchGl prints for a record, from a tile's arrays.

`format_into` runs the kernels on device tensors; `lines` puts "POS," in front of every site that has a line.

`fetch_file` is the other way in: a record file on disk (VCF text, gzip / bgzip'd, or BCF) through the program fetchgl_hip
(vcfgl_amd/csrc/misc), which takes any two characters for the genotype, as the tool does.
"""
import ctypes as C
import os
import subprocess

from . import _abi

FLOAT, TEXT = _abi.FETCHGL_FLOAT, _abi.FETCHGL_TEXT
LETTERS = "ACGT<"


def allele_codes(gt):
    """'AC' -> (0, 1); '<' is the unobserved allele (4)"""
    if len(gt) != 2 or gt[0] not in LETTERS or gt[1] not in LETTERS:
        raise ValueError("a genotype is two of A, C, G, T, <: %r" % (gt,))
    return LETTERS.index(gt[0]), LETTERS.index(gt[1])


def bound(n_samples, n_sites):
    return n_samples * n_sites * 48


def format_into(site_status, n_alleles, alleles2acgt, gl, a, b, value_mode, dst, offsets, workspace=None, max_genotypes=10,
                layout=_abi.VGL_LAYOUT_PLANES, stream=None, lib=None):
    """Formats one tile: device tensors site_status / n_alleles (int32 [n_sites]), alleles2acgt (int8 [n_sites][5]), gl (float32,
    n_sites * max_genotypes * n_samples values in `layout`), into dst (uint8) and offsets (int64 [n_sites + 1]).  Asynchronous on
    `stream`; returns the workspace tensor it used.  When offsets[n_sites] exceeds dst.numel() nothing was written."""
    import torch
    lib = lib or _abi.load_library()
    n_sites = int(site_status.numel())
    if n_sites == 0 or gl.numel() % (n_sites * max_genotypes):
        raise ValueError("gl must hold n_sites * max_genotypes * n_samples values")
    n = gl.numel() // (n_sites * max_genotypes)
    if offsets.numel() != n_sites + 1 or offsets.dtype != torch.int64 or dst.dtype != torch.uint8 or gl.dtype != torch.float32:
        raise ValueError("offsets is int64 [n_sites + 1], dst uint8, gl float32")
    need = lib.vgl_fetchgl_workspace_bytes(n, n_sites)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=gl.device)
    rc = lib.vgl_fetchgl_format_device(gl.device.index or 0, n, n_sites, max_genotypes, layout, site_status.data_ptr(), n_alleles.data_ptr(),
                                       alleles2acgt.data_ptr(), gl.data_ptr(), a, b, value_mode, dst.data_ptr() if dst.numel() else None,
                                       dst.numel(), offsets.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       C.c_void_p(stream) if stream else None)
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_fetchgl_format_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return workspace


def lines(pos, text, offsets):
    """the CSV bytes: "POS," and the site's text for every site whose text is not empty (pos: 1-based POS per site)"""
    raw = bytes(text)
    out = []
    for i in range(len(offsets) - 1):
        b, e = int(offsets[i]), int(offsets[i + 1])
        if e > b:
            out.append(b"%d," % int(pos[i]) + raw[b:e])
    return b"".join(out)


FETCHGL_PROGRAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "fetchgl_hip")


def fetch_file(path, gt, out=None, on_device=True, device=None, batch_records=None, messages=True, verbose=False, timeout=None, env=None,
               device_inflate=None, resident=None, resident_max_bytes=None, resident_bcf=None):
    """Runs fetchgl_hip -i `path` -gt `gt` [-o `out`] as a fresh child process and returns (returncode, stdout, stderr) as text;
    the CSV is in stdout, or in `out` when that is given.  on_device=False reads on the host and touches no GPU; on_device=True
    without a GPU fails (returncode 1): there is no fallback.  device_inflate=True inflates a BGZF file's members on the GPU
    (--device-inflate 1, also under on_device=False; any other file is read by zlib as without it); resident=True (with device_inflate
    and on_device) leaves the inflated text of a BGZF VCF in GPU memory and parses it there (--resident 1), resident_max_bytes bounds
    what it may take; resident_bcf=True (with resident) does the same for a BGZF BCF file, whose records are walked on the GPU
    (--resident-bcf 1).  A missing program is an error (build the package first)."""
    if not os.path.exists(FETCHGL_PROGRAM):
        raise FileNotFoundError("%s is not built (make -C vcfgl_amd/csrc all)" % FETCHGL_PROGRAM)
    cmd = [FETCHGL_PROGRAM, "-i", str(path), "-gt", str(gt), "--on-device", "1" if on_device else "0", "--messages", "1" if messages else "0"]
    if out is not None:
        cmd += ["-o", str(out)]
    if device is not None:
        cmd += ["--device", str(int(device))]
    if batch_records is not None:
        cmd += ["--batch-records", str(int(batch_records))]
    if device_inflate is not None:
        cmd += ["--device-inflate", "1" if device_inflate else "0"]
    if resident is not None:
        cmd += ["--resident", "1" if resident else "0"]
    if resident_max_bytes is not None:
        cmd += ["--resident-max-bytes", str(int(resident_max_bytes))]
    if resident_bcf is not None:
        cmd += ["--resident-bcf", "1" if resident_bcf else "0"]
    if verbose:
        cmd += ["--verbose", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr
