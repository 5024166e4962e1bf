"""The records of --depth inf, made on the device (vgl_inf.hip; include/vcfgl_hip.h, "the records of --depth inf"): what the
reference's simulate_record_true_values does, done to a tile's packed true genotypes -- the allele list of every site by descending
allele count, and per sample GL 0 / GP 1 / PL 0 at its true genotype, -inf / 0 / 255 at every other one.

`fill_into` runs the kernels on device tensors; `Simulator.true_values(1)` switches a context to them, so that `simulate`,
`simulate_device` and the text / BCF / stream paths deliver such records instead of simulated ones.
"""
import ctypes as C

from . import _abi

NO_SITE = 0x7FFFFFFF
GL_TRUE_BITS, GL_OTHER_BITS = 0x00000000, 0xFF800000        # 0.0f, -inf
PL_TRUE, PL_OTHER = 0, 255


def adds_unobserved(do_unobserved):
    return do_unobserved in (1, 2, 4, 5)


def max_alleles(do_unobserved):
    """the most alleles a site of a -doUnobserved `do_unobserved` run can have (vgl_max_alleles)"""
    return 5 if adds_unobserved(do_unobserved) else 4


def max_genotypes(do_unobserved):
    return 15 if adds_unobserved(do_unobserved) else 10


def workspace_bytes(n_samples, n_sites, lib=None):
    lib = lib or _abi.load_library()
    return lib.vgl_inf_workspace_bytes(n_samples, n_sites)


def fill_into(gt, site_status, n_alleles, n_alleles_obs, alleles2acgt, do_unobserved=1, gl=None, pl=None, gp=None, pl_u8=None, bad_site=None,
              workspace=None, layout=_abi.VGL_LAYOUT_PLANES, stream=None, lib=None):
    """Fills one tile: device tensors gt (uint8 [n_sites][n_samples]), site_status / n_alleles / n_alleles_obs (int32 [n_sites]),
    alleles2acgt (int8 [n_sites][5]) and whichever of gl, pl, gp, pl_u8 are given (max_genotypes(do_unobserved) planes per site).
    Asynchronous on `stream`; returns (bad_site, workspace): bad_site is an int32 tensor of one element, NO_SITE or the first site of
    the tile with a genotype that is not a pair of A, C, G, T."""
    import torch
    lib = lib or _abi.load_library()
    if gt.dtype != torch.uint8 or gt.dim() != 2 or not gt.is_contiguous():
        raise ValueError("gt is a contiguous uint8 [n_sites][n_samples]")
    n_sites, n_samples = int(gt.shape[0]), int(gt.shape[1])
    d = gt.device
    if bad_site is None:
        bad_site = torch.full((1,), NO_SITE, dtype=torch.int32, device=d)
    need = lib.vgl_inf_workspace_bytes(n_samples, n_sites)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=d)
    want = {"gl": torch.float32, "pl": torch.int32, "gp": torch.float32, "pl_u8": torch.uint8}
    given = {"gl": gl, "pl": pl, "gp": gp, "pl_u8": pl_u8}
    for k, t in given.items():
        if t is not None and t.dtype != want[k]:
            raise ValueError("%s must be %s" % (k, want[k]))
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = lib.vgl_inf_fill_device(d.index or 0, n_samples, n_sites, do_unobserved, max_genotypes(do_unobserved), max_alleles(do_unobserved), layout,
                                 gt.data_ptr(), site_status.data_ptr(), n_alleles.data_ptr(), n_alleles_obs.data_ptr(), alleles2acgt.data_ptr(),
                                 ptr(gl), ptr(pl), ptr(gp), ptr(pl_u8), bad_site.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                 C.c_void_p(stream) if stream else None)
    if rc != _abi.VGL_OK:
        raise RuntimeError("vgl_inf_fill_device: %d: %s" % (rc, lib.vgl_last_error().decode()))
    return bad_site, workspace
