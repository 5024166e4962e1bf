"""Model of the discordance tally (vgl_disc.hip, include/vcfgl_hip.h) in numpy: the rules every layer must agree with.

Per kept site (site_status >= 0) and sample:
  call missing  fmt_dp == 0, a true allele nibble outside 0 .. 3, or a site without a genotype of two A/C/G/T alleles
  call          lowest g < nG(site) with the smallest PL among the genotypes whose alleles both map to A/C/G/T (alleles2acgt)
  GQ            smallest PL over all g < nG(site) that is not 0, capped at 127; 127 when there is none  (gtDiscordance -doGQ 8)
  PL            a value outside [0, 255] (the int32 missing value included) counts as 255
  cell          true bases against called bases as unordered pairs
Table (int64): cell[sample][6][128] by GQ, callmis[sample], sites[2] = kept, skipped.
"""
import numpy as np

CELLS, NGQ = 6, 128
HOM_HOM_CONC, HOM_HOM_DISC, HET_HET_CONC, HET_HET_DISC, HOM_HET, HET_HOM = range(6)
PLANES, SAMPLE_MAJOR = 0, 1
INT32_MISSING = -(2 ** 31)


def table_len(n):
    return n * (CELLS * NGQ + 1) + 2


def views(table, n):
    k = n * CELLS * NGQ
    return table[:k].reshape(n, CELLS, NGQ), table[k:k + n], table[k + n:]


def genotype_alleles(nA):
    """(a[g], b[g]) of htslib's genotype order g = b (b + 1) / 2 + a, a <= b"""
    a, b = [], []
    for bb in range(nA):
        for aa in range(bb + 1):
            a.append(aa)
            b.append(bb)
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)


def classify(t0, t1, c0, c1):
    """cell of true bases (t0, t1) against called bases (c0, c1), arrays of equal shape"""
    thom, chom = t0 == t1, c0 == c1
    same = ((t0 == c0) & (t1 == c1)) | ((t0 == c1) & (t1 == c0))
    cell = np.where(thom & chom, np.where(t0 == c0, HOM_HOM_CONC, HOM_HOM_DISC),
                    np.where(~thom & ~chom, np.where(same, HET_HET_CONC, HET_HET_DISC), np.where(thom, HOM_HET, HET_HOM)))
    return cell.astype(np.int64)


def call_and_gq(P, codes):
    """P [..., nG] PL values, codes [nA] allele -> base (0 .. 3, anything else: not callable).  Returns (best g or -1, GQ) per row."""
    nA = len(codes)
    ga, gb = genotype_alleles(nA)
    P = np.asarray(P, dtype=np.int64)
    P = np.where((P < 0) | (P > 255), 255, P)
    ok = (np.asarray(codes) >= 0) & (np.asarray(codes) <= 3)
    valid = ok[ga] & ok[gb]
    Pv = np.where(valid, P, 256)
    best = np.where(Pv.min(axis=-1) == 256, -1, Pv.argmin(axis=-1))          # argmin: the lowest index of the minimum
    gq = np.minimum(np.where(P == 0, 255, P).min(axis=-1), 127)
    return best, gq


def tally(site_status, n_alleles, alleles2acgt, fmt_dp, pl, gt, layout=PLANES, table=None):
    """Adds one tile to `table` (a new one when None).  pl: [n_sites][G][n_samples] as the library lays it out in `layout`
    (uint8 or int32); gt: uint8 [n_sites][n_samples]."""
    site_status, n_alleles, fmt_dp, gt = (np.asarray(x) for x in (site_status, n_alleles, fmt_dp, gt))
    a2b = np.asarray(alleles2acgt).astype(np.int64)
    pl = np.asarray(pl)
    S, N = fmt_dp.shape
    if table is None:
        table = np.zeros(table_len(N), dtype=np.int64)
    cell, mis, sites = views(table, N)
    kept = site_status >= 0
    sites[0] += int(kept.sum())
    sites[1] += int((~kept).sum())
    t0, t1 = (gt & 15).astype(np.int64), (gt >> 4).astype(np.int64)
    for nA in range(0, 6):
        idx = np.nonzero(kept & (np.clip(n_alleles, 0, 5) == nA))[0]
        if not len(idx):
            continue
        n = len(idx)
        nG = nA * (nA + 1) // 2
        no_call = (fmt_dp[idx] == 0) | (t0[idx] > 3) | (t1[idx] > 3)
        if nG == 0:
            mis += n
            continue
        if layout == PLANES:
            P = pl[idx, :nG, :].transpose(0, 2, 1)
        else:
            P = pl[idx].reshape(n, -1)[:, :N * nG].reshape(n, N, nG)
        P = P.astype(np.int64)
        P = np.where((P < 0) | (P > 255), 255, P)
        ga, gb = genotype_alleles(nA)
        codes = a2b[idx, :nA]
        ok = (codes >= 0) & (codes <= 3)
        valid = ok[:, ga] & ok[:, gb]                                     # [n][nG]
        Pv = np.where(valid[:, None, :], P, 256)
        best = Pv.argmin(axis=2)
        no_call |= Pv.min(axis=2) == 256
        gq = np.minimum(np.where(P == 0, 255, P).min(axis=2), 127)
        rows = np.arange(n)[:, None]
        c0, c1 = codes[rows, ga[best]], codes[rows, gb[best]]
        cl = classify(t0[idx], t1[idx], c0, c1)
        mis += no_call.sum(axis=0)
        m = ~no_call
        samples = np.broadcast_to(np.arange(N)[None, :], (n, N))
        np.add.at(cell, (samples[m], cl[m], gq[m]), 1)
    return table


# ---- a truth file against a call file, GT read from the call file (what misc/gtDiscordance does) ---------------------------------
_BASE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _int_or_none(tok):
    try:
        return int(tok)
    except ValueError:
        return None


def record_gq(rec, s, has_gq_tag):
    """GQ of sample s of a call record: the GQ tag where the file declares one (127 for a record without it: a site called
    invariable), else the -doGQ 8 rule on PL"""
    if has_gq_tag:
        v = _int_or_none(rec.samples[s]["GQ"][0]) if "GQ" in rec.fmt_keys else None
        return 127 if v is None else v
    if "PL" not in rec.fmt_keys:
        return 127
    vals = [_int_or_none(x) for x in rec.samples[s]["PL"]]
    vals = [255 if (v is None or v < 0 or v > 255) else v for v in vals]
    nz = [v for v in vals if v != 0]
    return min(min(nz), 127) if nz else 127


def tally_vcf(truth, call, use_gq=True):
    """truth, call: vcfgl_amd.vcfio.VcfFile.  Sites are matched by (chrom, pos); a truth site the call file lacks is skipped.
    use_gq=False (-doGQ 0 reads no quality): every call goes to GQ 127."""
    n = len(truth.samples)
    table = np.zeros(table_len(n), dtype=np.int64)
    cell, mis, sites = views(table, n)
    has_gq = any(h.startswith("##FORMAT=<ID=GQ,") for h in call.header_lines)
    calls = {(r.chrom, r.pos0): r for r in call.records}
    for tr in truth.records:
        cr = calls.get((tr.chrom, tr.pos0))
        if cr is None:
            sites[1] += 1
            continue
        sites[0] += 1
        for s in range(n):
            a0, a1 = cr.gts[s]
            if a0 < 0 or a1 < 0:
                mis[s] += 1
                continue
            t = np.array([_BASE[tr.alleles[a][0]] for a in tr.gts[s]])
            c = np.array([_BASE[cr.alleles[a][0]] for a in (a0, a1)])
            gq = record_gq(cr, s, has_gq) if use_gq else 127
            assert 1 <= gq <= 127, gq
            cell[s, int(classify(t[:1], t[1:], c[:1], c[1:])[0]), gq] += 1
    return table


def ml_call(rec, s):
    """the model's call for sample s of a call record with a full PL vector: allele indices (a, b), or None"""
    nA = len(rec.alleles)
    vals = [_int_or_none(x) for x in rec.samples[s].get("PL", ["."])]
    if len(vals) != nA * (nA + 1) // 2 or any(v is None for v in vals):
        return None
    codes = [_BASE.get(a, 4) if len(a) == 1 else 4 for a in rec.alleles]
    best, _ = call_and_gq(np.array(vals), codes)
    if best < 0:
        return None
    ga, gb = genotype_alleles(nA)
    return int(ga[best]), int(gb[best])


def tally_records(truth, recs):
    """The model applied to a run's own files: `truth` is -printTruth's file, `recs` the simulated records (FORMAT/DP and PL), both
    vcfgl_amd.vcfio.VcfFile.  A truth site without a record was skipped by the run."""
    n = len(truth.samples)
    by_pos = {(r.chrom, r.pos0): r for r in recs.records}
    S = len(truth.records)
    status = np.zeros(S, dtype=np.int32)
    n_alleles = np.zeros(S, dtype=np.int32)
    a2b = np.full((S, 5), -1, dtype=np.int8)
    dp = np.zeros((S, n), dtype=np.int32)
    pl = np.full((S, 15, n), INT32_MISSING, dtype=np.int32)
    gt = np.zeros((S, n), dtype=np.uint8)
    for i, tr in enumerate(truth.records):
        for s in range(n):
            nib = [_BASE.get(tr.alleles[a], 15) if a >= 0 else 15 for a in tr.gts[s]]
            gt[i, s] = nib[0] | (nib[1] << 4)
        r = by_pos.get((tr.chrom, tr.pos0))
        if r is None:
            status[i] = -1
            continue
        n_alleles[i] = len(r.alleles)
        for k, a in enumerate(r.alleles):
            a2b[i, k] = _BASE.get(a, 4 if a.startswith("<") else -1)
        nG = len(r.alleles) * (len(r.alleles) + 1) // 2
        for s in range(n):
            d = _int_or_none(r.samples[s]["DP"][0])
            dp[i, s] = 0 if d is None else d
            vals = [_int_or_none(x) for x in r.samples[s]["PL"]]
            if len(vals) == nG:
                pl[i, :nG, s] = [INT32_MISSING if v is None else v for v in vals]
    return tally(status, n_alleles, a2b, dp, pl, gt, layout=PLANES)
