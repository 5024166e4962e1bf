"""Genotype calls and their discordance against the truth, tallied on the device (vgl_disc.hip; include/vcfgl_hip.h,
"genotype calls and their discordance").

The table is int64: cell[sample][6][128] indexed by GQ, then callmis[sample], then sites[2] = kept, skipped.
`tally_into` adds one tile of device tensors to a device table; `Simulator.discordance(1)` has a context tally every tile
it simulates; `format_table` prints a table in the layouts of the reference's misc/gtDiscordance (-doGQ 0, 3, 4, 5, 6).

`compare_files` is the other way in: a call file against a truth file, both on disk, through the program gtdiscordance_hip
(vcfgl_amd/csrc/misc), which covers every -doGQ mode, the per-call listings included.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi

N_CELLS, N_GQ = _abi.DISC_CELLS, _abi.DISC_GQ
GQ_ROWS = range(1, 130)                 # gtDiscordance prints k = 1 .. gq_arr_input_SIZE - 1 (GQ itself stops at 127)
MODES = (0, 3, 4, 5, 6)


def table_len(n_samples):
    return n_samples * (N_CELLS * N_GQ + 1) + 2


def split_table(table, n_samples=None):
    """views of a host table: (cell [N][6][128], callmis [N], sites [2])"""
    t = np.asarray(table if not hasattr(table, "cpu") else table.cpu().numpy())
    n = (t.size - 2) // (N_CELLS * N_GQ + 1) if n_samples is None else n_samples
    if t.dtype != np.int64 or t.ndim != 1 or t.size != table_len(n):
        raise ValueError("not a discordance table of %d samples" % n)
    k = n * N_CELLS * N_GQ
    return t[:k].reshape(n, N_CELLS, N_GQ), t[k:k + n], t[k + n:]


def new_table(n_samples, device):
    import torch
    return torch.zeros(table_len(n_samples), dtype=torch.int64, device=device)


def tally_into(tile, gt, table, layout=_abi.VGL_LAYOUT_PLANES, stream=None, lib=None):
    """Adds the calls of one tile (a Tile of device tensors with site_status, n_alleles, alleles2acgt, fmt_dp and pl_u8 or pl;
    pl_u8 is taken when the tile has both) against the true genotypes `gt` (uint8 device tensor [n_sites][n_samples]) to `table`
    (int64 device tensor of table_len(n_samples) elements).  Asynchronous on `stream`."""
    lib = lib or _abi.load_library()
    a = tile.arrays
    if tile.device is None:
        raise ValueError("tally_into takes device tensors")
    n_sites, n = tile.n_sites, tile.n_samples
    if tuple(gt.shape) != (n_sites, n) or not gt.is_contiguous() or table.numel() != table_len(n):
        raise ValueError("gt must be [n_sites][n_samples] and table table_len(n_samples) long")
    pl_u8 = a["pl_u8"].data_ptr() if "pl_u8" in a else None
    pl = a["pl"].data_ptr() if pl_u8 is None and "pl" in a else None
    rc = lib.vgl_disc_tally_device(table.device.index or 0, n, n_sites, tile.G, layout, a["site_status"].data_ptr(), a["n_alleles"].data_ptr(),
                                   a["alleles2acgt"].data_ptr(), a["fmt_dp"].data_ptr(), pl_u8, pl, gt.data_ptr(), table.data_ptr(),
                                   C.c_void_p(stream) if stream else None)
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_disc_tally_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return table


def _rate(num, den):
    # the reference divides doubles and prints %f: 0 / 0 is what x86-64 glibc prints for it
    return "-nan" if den == 0 else "%f" % (num / den)


def format_table(table, sample_names, mode=0):
    """The TSV text misc/gtDiscordance writes for -doGQ `mode` (0, 3, 4, 5 or 6; 7 and 8 equal 6: every call here has a GQ).
    Mode 0: nSitesTotal = kept + skipped sites, nSitesRetained = kept, nSitesinTrueNotCall = skipped."""
    if mode in (7, 8):
        mode = 6
    if mode not in MODES:
        raise ValueError("discordance table mode must be one of 0, 3, 4, 5, 6")
    cell, mis, sites = split_table(table, len(sample_names))
    cell = cell.astype(object)                          # Python integers: no width to think about
    n = len(sample_names)
    kept, skipped = int(sites[0]), int(sites[1])
    HH0, HH1, TT0, TT1, HT, TH = range(6)

    def row(c, k):                                      # the eight counts of a -doGQ 4 row from cells c [6][128]
        if k >= N_GQ:
            return [0] * 8
        d = [c[HH1][k], c[HT][k], c[TH][k], c[TT1][k]]
        return [sum(d)] + d + [c[HH0][k] + c[TT0][k], c[HH0][k], c[TT0][k]]

    out = []
    if mode == 0:
        for i in range(n):
            c = [int(sum(cell[i][j])) for j in range(N_CELLS)]
            compared = sum(c)
            disc = c[HH1] + c[TT1] + c[HT] + c[TH]
            total = kept + skipped
            miss = "-nan" if total == 0 else "%f" % (1.0 - compared / total)
            f = [sample_names[i], total, kept, compared, int(mis[i]), disc, skipped, compared - disc, miss, _rate(disc, compared),
                 _rate(compared - disc, compared), c[HH0], c[TT0], c[HH1], c[HT], c[TH], c[TT1]]
            f += [_rate(c[j], compared) for j in (HH0, TT0, HH1, HT, TH, TT1)]
            out.append("\t".join(str(x) for x in f))
    elif mode in (3, 4):
        tot = cell.sum(axis=0) if n else np.zeros((N_CELLS, N_GQ), dtype=object)
        for k in GQ_ROWS:
            r = row(tot, k)
            out.append("\t".join(str(x) for x in ([k, r[0], r[5]] if mode == 3 else [k] + r)))
    else:
        for i in range(n):
            compared = int(cell[i].sum())
            for k in GQ_ROWS:
                r = row(cell[i], k)
                out.append("\t".join(str(x) for x in ([i, k, r[0], r[5], compared] if mode == 5 else [i, k] + r + [compared])))
    return "".join(x + "\n" for x in out)


GTDISC_PROGRAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "gtdiscordance_hip")


def compare_files(truth, call, out, do_gq=0, per_site=False, on_device=True, device=None, batch_records=None, verbose=False,
                  timeout=None, env=None, device_inflate=None, bcf_direct=None, resident=None, resident_max_bytes=None):
    """Runs gtdiscordance_hip -t `truth` -i `call` -o `out` -doGQ `do_gq` [-perSite 1] as a fresh child process and returns
    (returncode, stdout, stderr) as text; stdout holds the -perSite lines, `out` the table or the -doGQ 1 / 2 listing.
    on_device=False compares on the host and touches no GPU; on_device=True without a GPU fails (returncode 1): there is no
    fallback.  device_inflate=True inflates the BGZF members of both files on the GPU (--device-inflate 1; any other file is read by
    zlib as without it), also under on_device=False.  bcf_direct=True judges a BCF file of the pair from its typed GT / GQ / PL vectors
    (--bcf-direct 1) and writes the same bytes as without it.  resident=True (--resident 1, with device_inflate and on_device) leaves
    each BGZF file of the pair in GPU memory once inflated -- VCF text, or BCF under bcf_direct -- so that only the records' heads
    come down and the batches read the files where they lie; resident_max_bytes bounds the inflated and compressed bytes of both
    files together (--resident-max-bytes; default: the GPU's free memory less 1 GiB).  A file that cannot be resident is read as
    without the flag; the bytes written are the same.  A missing program is an error (build the package first)."""
    if not os.path.exists(GTDISC_PROGRAM):
        raise FileNotFoundError("%s is not built (make -C vcfgl_amd/csrc all)" % GTDISC_PROGRAM)
    cmd = [GTDISC_PROGRAM, "-t", str(truth), "-i", str(call), "-o", str(out), "-doGQ", str(int(do_gq)), "-perSite", "1" if per_site else "0",
           "--on-device", "1" if on_device else "0"]
    if device is not None:
        cmd += ["--device", str(int(device))]
    if batch_records is not None:
        cmd += ["--batch-records", str(int(batch_records))]
    if device_inflate is not None:
        cmd += ["--device-inflate", "1" if device_inflate else "0"]
    if bcf_direct is not None:
        cmd += ["--bcf-direct", "1" if bcf_direct else "0"]
    if resident is not None:
        cmd += ["--resident", "1" if resident else "0"]
    if resident_max_bytes is not None:
        cmd += ["--resident-max-bytes", str(int(resident_max_bytes))]
    if verbose:
        cmd += ["--verbose", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr
