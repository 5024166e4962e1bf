"""Plain-Python statement of what the device decoder of BCF genotypes computes (include/vcfgl_hip.h, "the FORMAT/GT vectors of BCF
records"), and of what the host program's own reader (read_bcf of host/vcf_input.h + make_site of host/sites.h) computes for ANY record.

    value          a BCF2 typed integer: little endian, sign-extended, the int8 / int16 sentinels mapped to the int32 ones
    plain_sample   the per-sample rule: (a0, a1) of a sample inside the plain rule, None outside
    plain_record   the device's contract: (row, allelesum, BCFIN_OK) for a plain record, (None, None, BCFIN_HOST) else
    host_record    the host reader: the row and sum of any record it accepts ((int8_t) wrap of the allele index, a1 = a0 for a haploid
                   call), ModelDie where the program exits
    parse_bcf      a BCF2 file (raw or BGZF) as (samples, records); a record is a dict with pos, alleles and where its GT values lie
    file_rows      per record (pos, status, allelesum, row): what `vcfgl_hip --dump-gt FILE SOURCE 3` prints

Written from the issue's semantics, the BCF2 specification and the C++ reader; it shares no code with the package.
"""
import gzip

import numpy as np

from vcfin_model import ModelDie, _pack, allele_to_int

BCFIN_OK, BCFIN_HOST = 0, 1
MISSING, END = -2 ** 31, -2 ** 31 + 1                 # INT32_MIN, INT32_MIN + 1: what every width's sentinels become
WIDTH = {1: 1, 2: 2, 3: 4}                            # BCF type -> bytes (int8, int16, int32)
SENTINEL = {1: (-128, -127), 2: (-32768, -32767), 4: (MISSING, END)}


def value(buf, off, w):
    v = int.from_bytes(buf[off:off + w], "little", signed=True)
    missing, end = SENTINEL[w]
    return MISSING if v == missing else END if v == end else v


def encode(v, w):
    """the bytes of a value; "M" and "E" are the width's missing and end-of-vector sentinels"""
    if v == "M":
        v = SENTINEL[w][0]
    elif v == "E":
        v = SENTINEL[w][1]
    return int(v).to_bytes(w, "little", signed=True)


def plain_sample(vals, n_alleles):
    """vals: the sample's n >= 1 values (after `value`).  (a0, a1), or None when a used value is outside the plain rule"""
    v0 = vals[0]
    v1 = vals[1] if len(vals) >= 2 else END
    if v0 == END:
        return -1, -1                                # v1 is not used
    used = [v0] if v1 == END else [v0, v1]
    for v in used:
        if v < 0 or (v >> 1) - 1 >= n_alleles:       # the missing sentinel is the most negative value of all
            return None
    a0 = (v0 >> 1) - 1
    a1 = a0 if v1 == END else (v1 >> 1) - 1
    return a0, a1


def sample_values(buf, begin, gt_type, n, s):
    w = WIDTH[gt_type]
    return [value(buf, begin + (s * n + j) * w, w) for j in range(n)]


def describable(gt_type, n, n_alleles):
    return gt_type in WIDTH and n >= 1 and 1 <= n_alleles <= 5


def plain_record(buf, begin, gt_type, n, n_alleles, allele_map, n_samples):
    """The device's contract for the GT values at buf[begin:]."""
    if not describable(gt_type, n, n_alleles):
        return None, None, BCFIN_HOST
    row, total = np.empty(n_samples, np.uint8), 0
    for s in range(n_samples):
        g = plain_sample(sample_values(buf, begin, gt_type, n, s)[:2], n_alleles)      # values from the third on do not matter
        if g is None:
            return None, None, BCFIN_HOST
        total += max(g[0], 0) + max(g[1], 0)
        row[s] = _pack(g[0], g[1], allele_map)
    return row, total, BCFIN_OK


def _int8(x):
    x &= 0xFF
    return x - 256 if x >= 128 else x


def host_sample(vals):
    """read_bcf's rule for one sample: the values up to the first end-of-vector, (int8_t)((v >> 1) - 1) of the first two"""
    a = [-1, -1]
    for j, v in enumerate(vals):
        if v == END:
            break
        if j < 2:
            a[j] = _int8((v >> 1) - 1)
    if len(vals) == 1 or (len(vals) >= 2 and vals[1] == END):
        a[1] = a[0]
    return a[0], a[1]


def host_record(buf, begin, gt_type, n, n_alleles, allele_map, n_samples):
    """read_bcf + make_site for the GT values at buf[begin:]: (row, allelesum); ModelDie where the program exits."""
    if gt_type not in WIDTH and n_samples > 0:
        raise ModelDie("BCF: integer vector expected")
    row, total = np.empty(n_samples, np.uint8), 0
    for s in range(n_samples):
        a0, a1 = host_sample(sample_values(buf, begin, gt_type, n, s))
        for a in (a0, a1):
            if a >= n_alleles:
                raise ModelDie("GT allele index out of range")
        total += max(a0, 0) + max(a1, 0)
        row[s] = _pack(a0, a1, allele_map)
    return row, total


# ---- a BCF2 file ------------------------------------------------------------------------------------------------------------------
def _typed(buf, off):
    """the descriptor byte(s) at off: (type, n, offset behind them)"""
    b = buf[off]
    t, n, off = b & 15, b >> 4, off + 1
    if n == 15:
        t2, n2, off = _typed(buf, off)
        n = value(buf, off, WIDTH[t2])
        off += WIDTH[t2] * n2
    return t, n, off


def _typed_int(buf, off):
    t, n, off = _typed(buf, off)
    assert n == 1 and t in WIDTH
    return value(buf, off, WIDTH[t]), off + WIDTH[t]


def _attr(line, key):
    for opener in ("<", ","):
        a = line.find(opener + key + "=")
        if a >= 0:
            a += len(key) + 2
            e = min(i for i in (line.find(",", a), line.find(">", a)) if i >= 0)
            return line[a:e]
    return ""


def read_raw(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def parse_bcf(raw):
    """(samples, records) of the bytes of a BCF2 file.  A record: pos (1-based), alleles (bytes), gt_begin, gt_type, gt_n."""
    assert raw[:5] == b"BCF\x02\x02" or raw[:4] == b"BCF\x02"
    l_text = int.from_bytes(raw[5:9], "little")
    text = raw[9:9 + l_text].rstrip(b"\0\n").decode()
    lines = text.split("\n")
    dic, nd = {}, 0
    if not any(l.startswith("##FILTER=<") and _attr(l, "ID") == "PASS" for l in lines):
        dic[0], nd = "PASS", 1
    samples = []
    for l in lines:
        if not l.startswith("##"):
            if l.startswith("#"):
                samples = l.split("\t")[9:]
            continue
        if not l.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<")):
            continue
        ident, idx_s = _attr(l, "ID"), _attr(l, "IDX")
        idx = next((k for k, v in dic.items() if v == ident), -1)
        if idx < 0:
            idx = int(idx_s) if idx_s else nd
        dic[idx] = ident
        nd = max(nd, idx + 1)
    N, off, recs = len(samples), 9 + l_text, []
    while off < len(raw):
        l_shared, l_indiv = int.from_bytes(raw[off:off + 4], "little"), int.from_bytes(raw[off + 4:off + 8], "little")
        sh = off + 8
        pos0 = int.from_bytes(raw[sh + 4:sh + 8], "little", signed=True)
        nai, nfs = int.from_bytes(raw[sh + 16:sh + 20], "little"), int.from_bytes(raw[sh + 20:sh + 24], "little")
        n_allele, n_fmt = nai >> 16, nfs >> 24
        assert (nfs & 0xFFFFFF) == N
        p = sh + 24
        t, n, p = _typed(raw, p)                     # ID
        p += n
        alleles = []
        for _ in range(n_allele):
            t, n, p = _typed(raw, p)
            assert t == 7
            alleles.append(bytes(raw[p:p + n]))
            p += n
        rec = dict(pos=pos0 + 1, alleles=alleles, gt_begin=None)
        p = sh + l_shared
        for _ in range(n_fmt):
            key, p = _typed_int(raw, p)
            t, n, p = _typed(raw, p)
            w = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}.get(t, 0)
            if dic[key] == "GT":
                rec.update(gt_begin=p, gt_type=t, gt_n=n)
            p += w * n * N
        assert p <= sh + l_shared + l_indiv and rec["gt_begin"] is not None
        recs.append(rec)
        off = sh + l_shared + l_indiv
    return samples, recs


def allele_map_of(alleles, source):
    """make_site's ra[]; None where the program does not ask the device (allele_table refuses)"""
    if len(alleles) > 5 or (source == 0 and len(alleles) > 2):
        return None
    ra = [-1] * 5
    for i, a in enumerate(alleles):
        if source == 1:
            ra[i] = allele_to_int(a) if a else -1
            if ra[i] == -1:
                return None
        else:
            ra[i] = (a[0] if a else 0) - 48
            if ra[i] not in (0, 1):
                return None
    return ra


def file_rows(raw, source):
    """Per record of the bytes of a BCF file: (pos, status, allelesum, row) -- the row and sum by the host's rules, the status by the
    device's rule.  What `vcfgl_hip --dump-gt FILE SOURCE 3` prints (and, with -1 for every status, `... 0`)."""
    samples, recs = parse_bcf(raw)
    N, out = len(samples), []
    for r in recs:
        ra = allele_map_of(r["alleles"], source)
        if ra is None:
            raise ModelDie("alleles")
        _, _, st = plain_record(raw, r["gt_begin"], r["gt_type"], r["gt_n"], len(r["alleles"]), ra, N)
        row, total = host_record(raw, r["gt_begin"], r["gt_type"], r["gt_n"], len(r["alleles"]), ra, N)
        out.append((r["pos"], st, total, row))
    return out


def dump_text(rows, status=None):
    """status: what to print for every record's status instead of its own (--dump-gt ... 0 prints -1 for a BCF record)"""
    return "".join("%d %d %d %s\n" % (pos, st if status is None else status, total, bytes(row).hex()) for pos, st, total, row in rows)
