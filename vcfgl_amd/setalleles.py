"""A prescribed REF/ALT list for every record, applied on the device (vgl_setal.hip; include/vcfgl_hip.h, "a prescribed REF/ALT list"):
what the reference's misc/setAlleles does to a record file, done to a tile's arrays before any writer reads them.

`read_tsv` reads the tool's allele file (one `REF<TAB>ALT[,ALT...]` line per record), `build_table` turns its lines into the 8-byte
target entries of the ABI, `apply_into` runs the kernels on device tensors.  `Simulator.set_alleles(table)` relabels every tile of a
simulator.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi

LETTERS = "ACGT"
UNOBSERVED = 4
MAX_ALTS = 4
NO_SITE = 0x7FFFFFFF


def parse_line(line, nonref_name="<*>", where="line"):
    """'A\\tC,<*>' -> (0, 1, 4).  nonref_name is the run's own spelling of the unobserved allele; the other spelling is an error."""
    cols = line.rstrip("\r\n").split("\t")
    if len(cols) != 2 or not cols[0] or not cols[1]:
        raise ValueError("%s: expected REF<TAB>ALT[,ALT...]: %r" % (where, line))
    names = [cols[0]] + cols[1].split(",")
    if len(names) - 1 > MAX_ALTS:
        raise ValueError("%s: more than %d ALT alleles: %r" % (where, MAX_ALTS, line))
    codes = []
    for nm in names:
        if nm in LETTERS and len(nm) == 1:
            c = LETTERS.index(nm)
        elif nm == nonref_name:
            c = UNOBSERVED
        elif nm in ("<*>", "<NON_REF>"):
            raise ValueError("%s: the unobserved allele of this run is spelled %s, not %s" % (where, nonref_name, nm))
        else:
            raise ValueError("%s: unknown allele %r (A, C, G, T or %s)" % (where, nm, nonref_name))
        if c in codes:
            raise ValueError("%s: allele %s is named twice: %r" % (where, nm, line))
        codes.append(c)
    return tuple(codes)


def read_tsv(path, nonref_name="<*>"):
    """the allele lists of the file, one tuple of codes (0 .. 4) per line"""
    with open(path) as f:
        return [parse_line(ln, nonref_name, "%s:%d" % (path, k + 1)) for k, ln in enumerate(f)]


def build_table(targets):
    """[(0, 1, 4), ...] -> int8 [n][8]: [count, a0 .. a4 (-1 behind the count), 0, 0]"""
    t = np.zeros((len(targets), 8), np.int8)
    t[:, 1:6] = -1
    for i, codes in enumerate(targets):
        codes = [int(c) for c in codes]
        if not 2 <= len(codes) <= 5 or any(c < 0 or c > 4 for c in codes) or len(set(codes)) != len(codes):
            raise ValueError("site %d: a target is 2 .. 5 distinct alleles of 0 .. 4: %r" % (i, codes))
        t[i, 0] = len(codes)
        t[i, 1:1 + len(codes)] = codes
    return t


def workspace_bytes(n_samples, n_sites, max_genotypes, lib=None):
    lib = lib or _abi.load_library()
    return lib.vgl_setal_workspace_bytes(n_samples, n_sites, max_genotypes)


def apply_into(targets, site_status, n_alleles, alleles2acgt, n_samples, qs=None, fmt_dp=None, gl=None, pl=None, gp=None, pl_u8=None,
               bad_site=None, workspace=None, max_genotypes=10, max_alleles=4, layout=_abi.VGL_LAYOUT_PLANES, stream=None, lib=None):
    """Relabels one tile in place: device tensors targets (int8 [n_sites][8]), site_status / n_alleles (int32 [n_sites]), alleles2acgt
    (int8 [n_sites][5]), and whichever of qs, gl, pl, gp, pl_u8 are given (pl_u8 needs fmt_dp).  Asynchronous on `stream`; returns
    (bad_site, workspace): bad_site is an int32 tensor of one element, NO_SITE or the first refused site of the tile."""
    import torch
    lib = lib or _abi.load_library()
    n_sites = int(site_status.numel())
    d = site_status.device
    if bad_site is None:
        bad_site = torch.full((1,), NO_SITE, dtype=torch.int32, device=d)
    need = lib.vgl_setal_workspace_bytes(n_samples, n_sites, max_genotypes)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=d)
    want = {"qs": torch.float32, "fmt_dp": torch.int32, "gl": torch.float32, "pl": torch.int32, "gp": torch.float32, "pl_u8": torch.uint8}
    given = {"qs": qs, "fmt_dp": fmt_dp, "gl": gl, "pl": pl, "gp": gp, "pl_u8": pl_u8}
    for k, t in given.items():
        if t is not None and t.dtype != want[k]:
            raise ValueError("%s must be %s" % (k, want[k]))
    if targets.dtype != torch.int8 or targets.numel() != n_sites * 8:
        raise ValueError("targets is int8 [n_sites][8]")
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = lib.vgl_setal_apply_device(d.index or 0, n_samples, n_sites, max_genotypes, max_alleles, layout, targets.data_ptr(), site_status.data_ptr(),
                                    n_alleles.data_ptr(), alleles2acgt.data_ptr(), ptr(qs), ptr(fmt_dp), ptr(gl), ptr(pl), ptr(gp), ptr(pl_u8),
                                    bad_site.data_ptr(), workspace.data_ptr(), workspace.numel(), C.c_void_p(stream) if stream else None)
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_setal_apply_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return bad_site, workspace


SETALLELES_PROGRAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "setalleles_hip")


def set_file(path, alleles, out_prefix, mode="v", on_device=True, device=None, batch_records=None, threads=None, verbose=False, timeout=3600,
             env=None, device_inflate=None, resident=None, resident_max_bytes=None):
    """Runs setalleles_hip -i `path` -a `alleles` -O `mode` -o `out_prefix` as a fresh child process under `timeout` seconds
    (subprocess.TimeoutExpired when it runs out) and returns (returncode, stdout, stderr) as text.  The records are in `out_prefix`.vcf
    (mode v) or .vcf.gz (mode z) for VCF text input, in `out_prefix`.bcf (modes u, b) for BCF input.  on_device=True works BCF input on
    the GPU, fails without one and is refused for text input (returncode 1): there is no fallback; on_device=False works on the host
    and touches no GPU -- unless device_inflate=True, which inflates a BGZF input's members on the GPU (--device-inflate 1; any other
    file is read by zlib as without it).  resident=True (--resident 1; needs device_inflate=True and on_device=True, refused otherwise)
    keeps a BGZF file of BCF in GPU memory: the vectors are relabelled where they lie, the output records are assembled and, for mode b,
    compressed on the GPU; resident_max_bytes (--resident-max-bytes) bounds what the file and the batches' buffers may take there.  Any
    other file is worked as without the flag.  A missing program is an error (build the package first)."""
    if not os.path.exists(SETALLELES_PROGRAM):
        raise FileNotFoundError("%s is not built (make -C vcfgl_amd/csrc all)" % SETALLELES_PROGRAM)
    cmd = [SETALLELES_PROGRAM, "-i", str(path), "-a", str(alleles), "-O", str(mode), "-o", str(out_prefix), "--on-device", "1" if on_device else "0"]
    if device is not None:
        cmd += ["--device", str(int(device))]
    if batch_records is not None:
        cmd += ["--batch-records", str(int(batch_records))]
    if threads is not None:
        cmd += ["--threads", str(int(threads))]
    if device_inflate is not None:
        cmd += ["--device-inflate", "1" if device_inflate else "0"]
    if resident is not None:
        cmd += ["--resident", "1" if resident else "0"]
    if resident_max_bytes is not None:
        cmd += ["--resident-max-bytes", str(int(resident_max_bytes))]
    if verbose:
        cmd += ["--verbose", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr
