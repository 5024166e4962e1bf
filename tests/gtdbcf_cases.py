"""Inputs of the tests of gtdiscordance_hip --bcf-direct 1: a small BCF writer for typed GT / GQ / PL vectors (any width, any number of
values a sample, the missing and end-of-vector sentinels, fields of other types between them), the same records rendered as the VCF
text the program's text route makes of them -- which gives tests/gtdisc_model.py the expected result -- and the model's count of the
matched records that lie outside the plain rules (gm.plain_record on the rendered columns), which is what the program must hand to its
host reader, no more and no less."""
import random
import struct
import zlib

import gtdisc_model as gm

M, E = "M", "E"                          # the missing value and the end-of-vector of a typed vector
WIDTH = {1: 1, 2: 2, 3: 4}
_FMT = {1: "<b", 2: "<h", 3: "<i"}
_MIS = {1: -128, 2: -32768, 3: -2 ** 31}
INT32_MIN = -2 ** 31
KEYS = {"GT": 1, "GQ": 2, "PL": 3, "DP": 4}


def gt_value(allele, phased=0):
    """the BCF value of an allele index (-1: '.')"""
    return ((allele + 1) << 1) | phased


def enc(x, t):
    if x == M:
        x = _MIS[t]
    elif x == E:
        x = _MIS[t] + 1
    return struct.pack(_FMT[t], x)


def _typed(n, t):
    if n < 15:
        return bytes([(n << 4) | t])
    return bytes([0xF0 | t]) + (bytes([0x11, n]) if n < 128 else bytes([0x12]) + struct.pack("<h", n))


def typed_str(s):
    return _typed(len(s), 7) + s


class Rec:
    """a record: pos (1-based), alleles [str], fields [(key, BCF type, n, values)] -- values [N][n] of int / M / E for the types
    1 / 2 / 3, the raw bytes of the N vectors for any other type"""

    def __init__(self, pos, alleles, fields, rid="."):
        self.pos, self.alleles, self.fields, self.rid = pos, list(alleles), list(fields), rid


def header(samples, has_gq=True, has_pl=True, contig="chr1", length=2 ** 32 - 1):
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>', "##contig=<ID=%s,length=%d,IDX=0>" % (contig, length),
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype",IDX=1>']
    if has_gq:
        lines.append('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q",IDX=2>')
    if has_pl:
        lines.append('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p",IDX=3>')
    lines.append('##FORMAT=<ID=DP,Number=1,Type=Integer,Description="d",IDX=4>')
    return lines


def bcf_bytes(samples, recs, has_gq=True, has_pl=True):
    text = ("\n".join(header(samples, has_gq, has_pl) + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]) + "\n").encode() + b"\0"
    out = [b"BCF\x02\x02" + struct.pack("<I", len(text)) + text]
    n = len(samples)
    for r in recs:
        shared = struct.pack("<iiiIII", 0, r.pos - 1, 1, 0x7F800001, (len(r.alleles) << 16) | 0, (len(r.fields) << 24) | n)
        shared += typed_str(r.rid.encode()) + b"".join(typed_str(a.encode()) for a in r.alleles) + bytes([0x11, 0x00])
        indiv = b""
        for key, t, k, vals in r.fields:
            data = vals if isinstance(vals, bytes) else b"".join(enc(x, t) for v in vals for x in v)
            if not isinstance(vals, bytes):
                assert len(vals) == n and all(len(v) == k for v in vals), (key, k, n)
            indiv += bytes([0x11, KEYS[key]]) + _typed(k, t) + data
        out.append(struct.pack("<II", len(shared), len(indiv)) + shared + indiv)
    return b"".join(out)


def vector_offsets(samples, recs, key, has_gq=True, has_pl=True):
    """the file offset of every record's `key` vectors (to show that a test's vectors start at every offset mod 4)"""
    out = []
    for i, r in enumerate(recs):
        upto = bcf_bytes(samples, recs[:i], has_gq, has_pl)
        whole = bcf_bytes(samples, recs[:i] + [Rec(r.pos, r.alleles, r.fields[:[f[0] for f in r.fields].index(key) + 1], r.rid)], has_gq, has_pl)
        f = r.fields[[f[0] for f in r.fields].index(key)]
        out.append(len(whole) - WIDTH[f[1]] * f[2] * len(samples))
        assert len(upto) < out[-1]
    return out


def bgzf(data, block=4000):
    out = b""
    for at in list(range(0, len(data), block)) + [len(data)]:               # (the last member is the empty end-of-file block)
        chunk = data[at:at + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(chunk) + z.flush()
        out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out


# ---- the text a VCF writer gives GT, GQ and PL of these records ---------------------------------------------------------------------
def _wide(x):
    return INT32_MIN if x == M else INT32_MIN + 1 if x == E else x


def _num(x):
    return "." if x == INT32_MIN else "%d" % x


def columns(rec, n):
    """(FORMAT, the sample columns): the integer GT / GQ / PL fields alone (the last of a key counts), values up to the end-of-vector"""
    f = {}
    for key, t, k, vals in rec.fields:
        if t in WIDTH and key in ("GT", "GQ", "PL"):
            f[key] = (k, [[_wide(x) for x in v] for v in vals])
    keys = [k for k in ("GT", "GQ", "PL") if k in f]
    cols = []
    for s in range(n):
        tok = ""
        vals = f["GT"][1][s]
        j = 0
        while j < len(vals) and vals[j] != INT32_MIN + 1:
            x = vals[j]
            if j:
                tok += "|" if x & 1 else "/"
            tok += "." if (x >> 1) - 1 < 0 else "%d" % ((x >> 1) - 1)
            j += 1
        parts = [tok or "."]
        if "GQ" in f:
            v = f["GQ"][1][s]
            parts.append("." if not v or v[0] == INT32_MIN + 1 else _num(v[0]))
        if "PL" in f:
            v = f["PL"][1][s]
            v = v[:v.index(INT32_MIN + 1)] if INT32_MIN + 1 in v else v
            parts.append(",".join(_num(x) for x in v) or ".")
        cols.append(":".join(parts))
    return ":".join(keys), cols


def vcf_text(samples, recs, has_gq=True, has_pl=True):
    lines = header(samples, has_gq, has_pl)
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples))
    for r in recs:
        fmt, cols = columns(r, len(samples))
        lines.append("\t".join(["chr1", str(r.pos), ".", r.alleles[0], ",".join(r.alleles[1:]) or ".", ".", ".", ".", fmt] + cols))
    return "\n".join(lines) + "\n"


class Pair:
    """a truth and a call file, each as BCF (raw and BGZF) and as the text of the same records"""

    def __init__(self, d, name, samples, trecs, crecs, has_gq=True, has_pl=True):
        self.samples, self.trecs, self.crecs = samples, trecs, crecs
        p = lambda x: str(d / (name + x))
        self.t_bcf, self.c_bcf, self.t_vcf, self.c_vcf, self.t_bgzf, self.c_bgzf = p(".t.bcf"), p(".c.bcf"), p(".t.vcf"), p(".c.vcf"), p(".t.gz.bcf"), p(".c.gz.bcf")
        tb, cb = bcf_bytes(samples, trecs, False, False), bcf_bytes(samples, crecs, has_gq, has_pl)
        for path, data in ((self.t_bcf, tb), (self.c_bcf, cb), (self.t_bgzf, bgzf(tb)), (self.c_bgzf, bgzf(cb)),
                           (self.t_vcf, vcf_text(samples, trecs, False, False).encode()), (self.c_vcf, vcf_text(samples, crecs, has_gq, has_pl).encode())):
            with open(path, "wb") as f:
                f.write(data)

    def not_plain(self, do_gq):
        return not_plain(self.t_vcf, self.c_vcf, do_gq)


def not_plain(truth_vcf, call_vcf, do_gq):
    """the matched records, up to the one the run stops at, that gm.plain_record hands to the host rules: (count, records matched)"""
    th, ts, tr = gm.parse(truth_vcf)
    ch, cs, cr = gm.parse(call_vcf)
    n = len(ts)
    has_gq = any(h.startswith("##FORMAT=<ID=GQ,") for h in ch)
    amap = lambda al: sum((gm.BASE.get(al[a][0], 15) if a < len(al) else 15) << (4 * a) for a in range(16))
    by_pos = {}
    for rec in tr:
        by_pos.setdefault(rec[0], rec)
    count = matched = 0
    for pos, alleles, fmt, cols in cr:
        if pos not in by_pos:
            break
        _, talleles, tfmt, tcols = by_pos[pos]
        gqi = fmt.index("GQ") if "GQ" in fmt else -1
        pli = fmt.index("PL") if "PL" in fmt else -1
        if do_gq == 0:
            mode = gm.GQ_NONE
        elif do_gq <= 6:
            if gqi < 0:
                break
            mode = gm.GQ_TAG
        elif do_gq == 7 or has_gq:
            mode = gm.GQ_TAG if gqi >= 0 else gm.GQ_MAX
        else:
            if pli < 0 or len(alleles) > 5:
                break
            mode = gm.GQ_PL
        matched += 1
        v = gm.plain_record("\t".join(tcols), "\t".join(cols), n, (tfmt.index("GT"), len(talleles), amap(talleles)),
                            (fmt.index("GT"), gqi, pli, len(alleles), amap(alleles)), mode)
        count += v is None
    return count, matched


# ---- records from the text generator of tests/gtdisc_model.py -----------------------------------------------------------------------
def from_text(path, types=(1, 1, 2), gt_n=2, odd_kind="wide"):
    """The records of a VCF text file as typed fields of the BCF types `types` (GT, GQ / DP, PL).  BCF holds numbers, not tokens, so
    the generator's odd token (an allele index written with three digits, '005') would vanish: the sample that carries it gets a
    call outside the plain rules that the host rules still read -- './1xx', a missing call beside an index of three digits."""
    header, samples, recs = gm.parse(path)
    out = []
    for pos, alleles, fmt, cols in recs:
        fields = []
        for k, key in enumerate(fmt):
            toks = [c.split(":")[k] for c in cols]
            if key == "GT":
                vals = []
                for tok in toks:
                    sep = "|" if "|" in tok else "/"
                    a, b = tok.split(sep)
                    if len(a) == 3 or len(b) == 3:
                        v = [gt_value(-1), gt_value(100 + int(b if b != "." else a), sep == "|")]
                    else:
                        v = [gt_value(-1 if a == "." else int(a)), gt_value(-1 if b == "." else int(b), sep == "|")]
                    vals.append(v + [E] * (gt_n - 2))
                wide = max(x for v in vals for x in v if x != E) > 127          # (a writer widens the record's vectors to int16 then)
                fields.append(("GT", max(types[0], 2) if wide else types[0], gt_n, vals))
            elif key in ("GQ", "DP"):
                fields.append((key, types[1], 1, [[M if tok == "." else int(tok)] for tok in toks]))
            elif key == "PL":
                rows = [[M if x == "." else int(x) for x in tok.split(",")] for tok in toks]
                width = max(len(r) for r in rows)
                fields.append(("PL", types[2], width, [r + [E] * (width - len(r)) for r in rows]))
        out.append(Rec(pos, alleles, fields))
    return samples, out


def pair_from_generator(d, name, n, n_records, fmt, seed, odd_share=0.0, invariant=False, first_pos=8, types=(1, 1, 2), gt_n=2):
    """gm.write_pair's records as a Pair; the call file's header declares GQ / PL as the text file's does"""
    t, c = str(d / (name + ".gen.t.vcf")), str(d / (name + ".gen.c.vcf"))
    gm.write_pair(t, c, n, n_records, fmt, seed=seed, first_pos=first_pos, invariant=invariant, odd_share=odd_share)
    samples, trecs = from_text(t, types=types, gt_n=gt_n)
    _, crecs = from_text(c, types=types, gt_n=gt_n)
    keys = fmt.split(":")
    return Pair(d, name, samples, trecs, crecs, has_gq="GQ" in keys, has_pl="PL" in keys)


def simple_pair(d, name, n, n_records, seed, call_fields, nal=4, first_pos=1, ids=None, alleles=None, truth_type=1):
    """all-plain truth records (int8 pairs) and call records whose fields call_fields(rnd, record index, truth alleles [n][2], nal)
    gives; `ids` / `alleles`: the ID and the allele strings of record i (odd lengths move the vectors through every offset mod 4)"""
    rnd = random.Random(seed)
    samples = ["s%d" % i for i in range(n)]
    trecs, crecs = [], []
    for i in range(n_records):
        al = alleles(i) if alleles else ["A", "C", "G", "T", "AA"][:nal]
        tg = [[rnd.randrange(min(len(al), 4)), rnd.randrange(min(len(al), 4))] for _ in range(n)]
        rid = ids(i) if ids else "."
        trecs.append(Rec(first_pos + i, al, [("GT", truth_type, 2, [[gt_value(a), gt_value(b, rnd.randrange(2))] for a, b in tg])], rid))
        crecs.append(Rec(first_pos + i, al, call_fields(rnd, i, tg, len(al)), rid))
    return samples, trecs, crecs
