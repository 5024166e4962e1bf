"""A plain Python model of the host writer's pileup columns (vcfgl_hip -printPileup 1, host/tile_writer.h TileWriter::pileup_line): what follows
the prefix chrom "\\t" pos "\\t" ref on every line, from a tile's site_status, DP and read dump and the quality rule.

    text, offsets = render(site_status, dp, reads)                 # each read's own score + 33
    text, offsets = render(site_status, dp, reads, qual=q)         # q: one score byte for every read (--adjust-qs 4, --error-qs 0 / 1)
    text, offsets = render(site_status, dp, reads, qual=scores)    # scores [read_capacity, n_sites, N]: adjusted scores (--error-qs 2)

dp is [n_sites, N], reads [read_capacity, n_sites, N] (uint8: score << 2 | base).  A VGL_SITE_SKIP_EMPTY site has no text."""
import math

import numpy as np

SITE_SKIP_EMPTY = -4
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def column(dp, reads_col, qual=None):
    """one sample's column with its leading tab: reads_col = the sample's read bytes (at least dp of them)"""
    if dp == 0:
        return b"\t0\t*\t*"
    r = np.asarray(reads_col[:dp], dtype=np.uint8)
    bases = ACGT[r & 3].tobytes()
    if qual is None:
        quals = ((r >> 2) + 33).astype(np.uint8).tobytes()
    elif np.isscalar(qual):
        quals = bytes([int(qual)]) * dp
    else:
        quals = ((np.asarray(qual[:dp], dtype=np.int64) + 33) & 0xFF).astype(np.uint8).tobytes()
    return b"\t%d\t" % dp + bases + b"\t" + quals


def render(site_status, dp, reads, qual=None):
    """(bytes, offsets [n_sites + 1]): the device formatter's output for a tile"""
    site_status = np.asarray(site_status)
    dp = np.asarray(dp)
    S, N = dp.shape
    out, offsets = [], [0]
    for i in range(S):
        if site_status[i] == SITE_SKIP_EMPTY:
            offsets.append(offsets[-1])
            continue
        parts = []
        for s in range(N):
            q = qual if qual is None or np.isscalar(qual) else qual[:, i, s]
            parts.append(column(int(dp[i, s]), reads[:, i, s], q))
        parts.append(b"\n")
        out.append(b"".join(parts))
        offsets.append(offsets[-1] + len(out[-1]))
    return b"".join(out), np.array(offsets, dtype=np.int64)


def column_bound(read_capacity):
    """the longest column of a sample whose depth is at most read_capacity"""
    return max(6, 3 + len(str(read_capacity)) + 2 * read_capacity)


def adjusted_score(ep, adjust_by=0.499, bins=None):
    """the host's --adjust-qs 4 score of one read under --error-qs 2 (host_errprob_to_qs): -1 for an error probability of 0 or 1"""
    if ep == 0.0 or ep == 1.0:
        aq = -1
    else:
        aq = int(-10.0 * math.log10(ep) + adjust_by)
    if bins:
        for lo, hi, v in bins:
            if lo <= aq <= hi:
                return v
        raise ValueError(f"no bin for {aq}")
    return min(aq, 63)


def parse_lines(text):
    """[(chrom, pos, ref, [(dp, bases, quals)])] of a pileup file's text"""
    rows = []
    for line in text.split("\n"):
        if not line:
            continue
        f = line.split("\t")
        rows.append((f[0], int(f[1]), f[2], [(int(f[3 + 3 * k]), f[4 + 3 * k], f[5 + 3 * k]) for k in range((len(f) - 3) // 3)]))
    return rows


def arrays_of(rows):
    """(dp [S, N], reads [R, S, N]) that a pileup's lines were printed from (each read's own score: (ord(q) - 33) << 2 | base)"""
    S, N = len(rows), len(rows[0][3])
    R = max(1, max(n for _, _, _, smp in rows for n, _, _ in smp))
    dp = np.zeros((S, N), dtype=np.int32)
    reads = np.full((R, S, N), 0xFF, dtype=np.uint8)
    for i, (_, _, _, smp) in enumerate(rows):
        for s, (n, bases, quals) in enumerate(smp):
            dp[i, s] = n
            for r in range(n):
                reads[r, i, s] = ((ord(quals[r]) - 33) << 2) | "ACGT".index(bases[r])
    return dp, reads
