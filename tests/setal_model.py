"""A numpy float32 model of the reference's misc/setAlleles, on the arrays of a tile (the specification of vgl_setal.hip).

For a record with alleles old (codes 0 .. 4 = A, C, G, T, unobserved) and a target list new:
  old2new[a]      the index of old allele a in new, or -1
  oldgt2newgt[g]  alleles2gt(old2new[a1], old2new[a2]) for g = a2 (a2 + 1) / 2 + a1 when both are >= 0
  QS              new[old2new[a]] = old[a]
  GL, PL, GP      per sample new[oldgt2newgt[g]] = old[g], then
                    GL: a NaN among the new values -> left as scattered; else minus the float maximum
                    PL: INT32_MIN among them -> left; else (int32)((float)pl - (float)min)
                    GP: a NaN -> left; else divided by the float sum taken in ascending new-genotype order
  pl_u8           missing iff fmt_dp == 0 (left as scattered); else v - min
A target with an allele the record does not have is the tool's undefined case: `relabel_tile` reports the site in `bad` and leaves it.
Everything is computed on 32-bit patterns so that NaN payloads survive; arithmetic is numpy float32 (IEEE, no fused operation).
"""
import numpy as np

PLANES, SAMPLE_MAJOR = 0, 1
FLOAT_MISSING = np.uint32(0x7F800001)
INT32_MISSING = np.uint32(0x80000000)
NO_SITE = 0x7FFFFFFF
KINDS = ("gl", "pl", "gp", "pl_u8")


def alleles2gt(a, b):
    return b * (b + 1) // 2 + a if b > a else a * (a + 1) // 2 + b


def n_gt(n):
    return n * (n + 1) // 2


def allele_map(old, new):
    return [new.index(a) if a in new else -1 for a in old]


def genotype_map(old2new):
    n = len(old2new)
    m = []
    for a2 in range(n):
        for a1 in range(a2 + 1):
            n1, n2 = old2new[a1], old2new[a2]
            m.append(alleles2gt(n1, n2) if n1 >= 0 and n2 >= 0 else -1)
    return m


def is_nan_bits(b):
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def scatter(old_vals, g2g, n_new_gt, fill):
    """old_vals [nG_old, N] (any dtype) -> [n_new_gt, N]; new genotypes no old one maps to hold `fill`"""
    out = np.full((n_new_gt,) + old_vals.shape[1:], fill, dtype=old_vals.dtype)
    for g, h in enumerate(g2g):
        if h >= 0:
            out[h] = old_vals[g]
    return out


def norm_gl(bits):
    """bits uint32 [n, N] in new order -> normalised copy"""
    out = bits.copy()
    miss = is_nan_bits(bits).any(axis=0)
    f = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        mx = np.full(bits.shape[1], -np.inf, np.float32)
        for g in range(bits.shape[0]):
            mx = np.where(f[g] > mx, f[g], mx)
        res = (f - mx[None, :]).astype(np.float32).view(np.uint32)
    out[:, ~miss] = res[:, ~miss]
    return out


def norm_pl(bits):
    out = bits.copy()
    miss = (bits == INT32_MISSING).any(axis=0)
    v = bits.view(np.int32).astype(np.float32)
    mn = np.full(bits.shape[1], np.inf, np.float32)
    for g in range(bits.shape[0]):
        mn = np.where(v[g] < mn, v[g], mn)
    keep = ~miss
    res = (v[:, keep] - mn[None, keep]).astype(np.float32).astype(np.int32).view(np.uint32)
    out[:, keep] = res
    return out


def norm_gp(bits):
    out = bits.copy()
    miss = is_nan_bits(bits).any(axis=0)
    f = bits.view(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.zeros(bits.shape[1], np.float32)
        for g in range(bits.shape[0]):
            s = (s + f[g]).astype(np.float32)
        res = (f / s[None, :]).astype(np.float32).view(np.uint32)
    out[:, ~miss] = res[:, ~miss]
    return out


def norm_u8(vals, missing):
    out = vals.copy()
    keep = ~missing
    v = vals[:, keep].astype(np.int32)
    out[:, keep] = (v - v.min(axis=0)[None, :]).astype(np.uint8)
    return out


def relabel_record(old, new, qs=None, gl=None, pl=None, gp=None, pl_u8=None, dp=None):
    """One record.  old / new: lists of allele codes.  qs: float32 [>= len(old)]; gl, gp: uint32 bits [nG_old, N]; pl: uint32 bits of
    int32 [nG_old, N]; pl_u8: uint8 [nG_old, N] with dp int32 [N].  Returns a dict of the new arrays ([nG_new, N]; qs [len(new)])."""
    o2n = allele_map(old, new)
    g2g = genotype_map(o2n)
    nG = n_gt(len(new))
    r = {}
    if qs is not None:
        q = np.zeros(len(new), np.float32)
        for a, j in enumerate(o2n):
            if j >= 0:
                q[j] = qs[a]
        r["qs"] = q
    if gl is not None:
        r["gl"] = norm_gl(scatter(gl, g2g, nG, FLOAT_MISSING))
    if pl is not None:
        r["pl"] = norm_pl(scatter(pl, g2g, nG, INT32_MISSING))
    if gp is not None:
        r["gp"] = norm_gp(scatter(gp, g2g, nG, FLOAT_MISSING))
    if pl_u8 is not None:
        r["pl_u8"] = norm_u8(scatter(pl_u8, g2g, nG, np.uint8(255)), dp == 0)
    return r


def site_view(x, i, G, N, nG, layout):
    """the [nG, N] values of site i of a flat tile array (a copy)"""
    slab = x.reshape(-1)[i * G * N:(i + 1) * G * N]
    return slab[:nG * N].reshape(nG, N).copy() if layout == PLANES else slab[:N * nG].reshape(N, nG).T.copy()


def site_store(x, i, G, N, vals, layout, fill):
    flat = x.reshape(-1)
    nG = vals.shape[0]
    if layout == PLANES:
        flat[i * G * N:i * G * N + nG * N] = vals.reshape(-1)
        flat[i * G * N + nG * N:(i + 1) * G * N] = fill
    else:
        flat[i * G * N:i * G * N + N * nG] = vals.T.reshape(-1)


def relabel_tile(targets, site_status, n_alleles, a2b, N, G, A, layout, qs=None, fmt_dp=None, gl=None, pl=None, gp=None, pl_u8=None):
    """The whole tile, on copies.  targets: list of tuples of codes (or None for "keep").  gl / gp: uint32 bit arrays, pl: int32,
    pl_u8: uint8, flat or shaped, n_sites * G * N values in `layout`.  Returns (dict of new arrays, first refused site or NO_SITE).
    VGL_LAYOUT_SAMPLE_MAJOR: only the first N * nG_new values of a slab are defined; the rest keeps the input's values here, and the
    caller compares with `defined_mask`."""
    S = len(site_status)
    out = {"n_alleles": np.array(n_alleles, np.int32).copy(), "a2b": np.array(a2b, np.int8).copy()}
    arrays = {"gl": gl, "pl": pl, "gp": gp, "pl_u8": pl_u8}
    fills = {"gl": FLOAT_MISSING, "pl": np.int32(-2 ** 31), "gp": FLOAT_MISSING, "pl_u8": np.uint8(255)}
    for k, x in arrays.items():
        if x is not None:
            out[k] = np.array(x).reshape(-1).copy()
    if qs is not None:
        out["qs"] = np.array(qs, np.float32).reshape(S, A).copy()
    bad = NO_SITE
    for i in range(S):
        if site_status[i] < 0:
            continue
        nA = int(n_alleles[i])
        old = [int(c) for c in a2b[i][:nA]]
        new = [int(c) for c in targets[i]]
        ok = (1 <= nA <= 5 and 2 <= len(new) <= 5 and len(set(new)) == len(new) and all(0 <= c <= 4 and c in old for c in new)
              and n_gt(nA) <= G and n_gt(len(new)) <= G and len(new) <= A)
        if not ok:
            bad = min(bad, i)
            continue
        nGo = n_gt(nA)
        kw = {}
        for k, x in arrays.items():
            if x is not None:
                v = site_view(np.array(x), i, G, N, nGo, layout)
                kw[k] = v.view(np.uint32) if k == "pl" else v
        if pl_u8 is not None:
            kw["dp"] = np.array(fmt_dp).reshape(S, N)[i]
        if qs is not None:
            kw["qs"] = out["qs"][i].copy()
        r = relabel_record(old, new, **kw)
        for k in KINDS:
            if k in r:
                v = r[k].view(np.int32) if k == "pl" else r[k]
                site_store(out[k], i, G, N, v, layout, fills[k])
        if qs is not None:
            out["qs"][i][:len(new)] = r["qs"]
        out["n_alleles"][i] = len(new)
        out["a2b"][i] = new + [-1] * (5 - len(new))
    return out, bad


def defined_mask(site_status, n_alleles_new, N, G, layout):
    """bool [n_sites * G * N]: the values of a FORMAT array the contract defines (sample-major: the record's array at the head of its slab)"""
    S = len(site_status)
    m = np.ones((S, G * N), bool)
    if layout == SAMPLE_MAJOR:
        for i in range(S):
            m[i, N * n_gt(int(n_alleles_new[i])):] = False
    return m.reshape(-1)
