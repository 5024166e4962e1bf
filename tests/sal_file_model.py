"""Plain Python model of setalleles_hip (vcfgl_amd/csrc/misc: the reference's misc/setAlleles on a record file) and a generator of
record files for it.  The model builds on setal_model (the maps, the three normalisations), vcftext_model (htslib's number text) and
fgl_file_model (the float token grammar, the BGZF writer).  It covers both families: VCF text (run_text) and BCF (run_bcf, with an encoder that writes records the way htslib does).

Rules (vcfgl_amd/csrc/misc/sal_core.h, setal_main.cpp):
    alleles        names compared whole; old2new[a] from the TSV line of the record, oldgt2newgt as the tool builds it, values scattered
                   in ascending old genotype order
    stops, early   a record with more than 5 alleles, a TSV name the record lacks, a QS count other than the allele count, a line count
                   other than the record count: before any output
    QS             new[old2new[a]] = old[a], reprinted by the number writer
    values         a sample column that ends before a field, or whose field is '.', is one missing value; the old vector is the tokens
                   and then end-of-vector up to nG_old; a text value is strtod / strtol and a cast
    GL, GP         any NaN among the new values: the first becomes the missing pattern, nothing else changes; else max subtracted /
                   divided by the ascending float sum; a NaN the arithmetic makes is 0x7FC00000
    PL             INT32_MIN among the new values: as gathered; else (int32)((float)pl - (float)min), all end-of-vector -> zeros
    stops, late    in this order for a record: a token strtod / strtol does not take whole (first in column, then FORMAT order), a column
                   count other than the header's, a field with more values than nG_old, a PL sample whose cast would overflow
                   (end-of-vector beside ordinary values, or a difference of 2^31 and more); the records before it are written
    text           values up to the first end-of-vector, '.' for missing and for an empty list; untouched fields are their bytes; a field
                   the column ended before stays away
`redone` counts the records that hold a token outside the device grammar (fgl_file_model.in_grammar; PL: an optional sign and 1 .. 10
digits inside int32, or '.')."""
import gzip
import re
import struct

import numpy as np

import bcf_reader
import fgl_file_model as ff
import setal_model as sm
import vcftext_model as vt

F_MISSING, F_END, QNAN = 0x7F800001, 0x7F800002, 0x7FC00000
I_MISSING, I_END = -2 ** 31, -2 ** 31 + 1
TAGS = ("GL", "PL", "GP")
CONTAINERS = ("vcf", "gz", "bgz")
_PL_DEV = re.compile(r"[+-]?[0-9]{1,10}\Z")
_PL_HOST = re.compile(r"[ \t\n\v\f\r]*[+-]?[0-9]+\Z")


def pl_in_grammar(tok):
    return tok == "." or (bool(_PL_DEV.match(tok)) and -2 ** 31 <= int(tok) <= 2 ** 31 - 1)


def pl_value(tok):
    """the int32 strtol reads; None: not taken whole, or outside int32"""
    if tok == ".":
        return I_MISSING
    if not _PL_HOST.match(tok):
        return None
    v = int(tok)
    return v if -2 ** 31 <= v <= 2 ** 31 - 1 else None


def float_value(tok):
    return F_MISSING if tok == "." else ff.token_bits(tok)


def norm_float(bits, gp):
    """bits uint32 [n, N] in the new order"""
    nan = sm.is_nan_bits(bits)
    miss = nan.any(axis=0)
    out = (sm.norm_gp if gp else sm.norm_gl)(bits)
    made = sm.is_nan_bits(out) & ~miss[None, :]
    out[made] = QNAN
    first = nan.argmax(axis=0)
    for s in np.nonzero(miss)[0]:
        out[first[s], s] = F_MISSING
    return out


def norm_pl(bits):
    """-> (new bits, True when a sample's cast would overflow)"""
    v = bits.view(np.int32)
    miss = (v == I_MISSING).any(axis=0)
    end = v == I_END
    mix = end.any(axis=0) & ~end.all(axis=0) & ~miss
    f = v.astype(np.float32)
    d = (f - f.min(axis=0)[None, :]).astype(np.float32)
    over = (d >= np.float32(2147483648.0)).any(axis=0) & ~miss
    if (mix | over).any():
        return bits, True
    out = bits.copy()
    out[:, ~miss] = d[:, ~miss].astype(np.int64).astype(np.int32).view(np.uint32)
    return out, False


class Result:
    def __init__(self):
        self.out = ""                      # the decompressed output: header and the records up to a stop
        self.stop = None                   # (kind, POS)
        self.redone = 0
        self.records = 0

    @property
    def returncode(self):
        return 1 if self.stop else 0


def early_stop(text, targets):
    """the stop the nine-column pass finds, or None"""
    recs = [ln.split("\t") for ln in text.split("\n") if ln and ln[0] != "#"]
    for i, f in enumerate(recs):
        if i >= len(targets):
            break
        pos = int(f[1])
        alleles = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        if len(alleles) > 5:
            return ("alleles", pos)
        for a in targets[i]:
            if a not in alleles:
                return ("lacks", pos)
        for kv in f[7].split(";"):
            if kv.startswith("QS=") and len(kv[3:].split(",")) != len(alleles):
                return ("qs", pos)
    if len(recs) != len(targets):
        return ("count", None)
    return None


def relabel_columns(keys, where, cols, N, n_old, g2g, nGn):
    """the sample columns of one record -> (a token outside the device grammar, the stop kind or None, {tag: new bits [nGn, N]})"""
    nGo = sm.n_gt(n_old)
    # the old vectors, in the order the program reads tokens
    old = {t: np.empty((nGo, N), np.uint32) for t in where}
    odd = bad = many = False
    split_cols = [c.split(":") for c in cols]
    for s, sub in enumerate(split_cols[:N]):
        for k, key in enumerate(keys):
            if key not in where or where[key] != k:
                continue
            toks = sub[k].split(",") if k < len(sub) else ["."]
            many = many or len(toks) > nGo
            for g in range(nGo):
                if g >= len(toks):
                    v = I_END if key == "PL" else F_END
                elif key == "PL":
                    odd = odd or not pl_in_grammar(toks[g])
                    v = pl_value(toks[g])
                else:
                    odd = odd or not ff.in_grammar(toks[g])
                    v = float_value(toks[g])
                if v is None:
                    bad, v = True, 0
                old[key][g, s] = v & 0xFFFFFFFF
    stop = "token" if bad else "columns" if len(cols) != N else "many" if many else None
    new = {}
    if not stop:
        for t in where:
            g = sm.scatter(old[t], g2g, nGn, 0)
            if t == "PL":
                new[t], over = norm_pl(g)
                if over:
                    stop = "pl"
            else:
                new[t] = norm_float(g, t == "GP")
        # (GL before PL before GP: the overflow of PL is the only stop of this stage)
    return odd, stop, new


def run_text(text, targets):
    """the run of setalleles_hip on VCF text; targets: a list of name lists (REF first), one per record"""
    res = Result()
    res.stop = early_stop(text, targets)
    if res.stop:
        return res
    lines = text.split("\n")
    names = [ln for ln in lines if ln.startswith("#CHROM")]
    N = max(len(names[0].split("\t")) - 9, 0)
    out = [ln + "\n" for ln in lines if ln.startswith("#")]
    i = -1
    for ln in lines:
        if not ln or ln[0] == "#":
            continue
        i += 1
        f = ln.split("\t")
        pos, tgt = int(f[1]), targets[i]
        alleles = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        o2n = sm.allele_map(alleles, tgt)
        g2g = sm.genotype_map(o2n)
        nGo, nGn = sm.n_gt(len(alleles)), sm.n_gt(len(tgt))
        info = []
        for kv in f[7].split(";"):
            if kv.startswith("QS="):
                old = kv[3:].split(",")
                new = [None] * len(tgt)
                for a, j in enumerate(o2n):
                    if j >= 0:
                        new[j] = vt.fmt_float_bits(float_value(old[a]))
                kv = "QS=" + ",".join(new)
            info.append(kv)
        fixed = f[:3] + [tgt[0], ",".join(tgt[1:])] + f[5:7] + [";".join(info)] + f[8:9]
        keys = f[8].split(":") if len(f) > 8 else []
        where = {t: keys.index(t) for t in TAGS if t in keys}
        cols = f[9:]
        if not where or not cols:
            out.append("\t".join(fixed + cols) + "\n")
            res.records += 1
            continue
        odd, stop, new = relabel_columns(keys, where, cols, N, len(alleles), g2g, nGn)
        res.redone += 1 if odd else 0
        split_cols = [c.split(":") for c in cols]
        if stop:
            res.stop = (stop, pos)
            break
        new_cols = []
        for s, sub in enumerate(split_cols):
            parts = []
            for k, field in enumerate(sub):
                key = keys[k] if k < len(keys) else None
                if key in where and where[key] == k:
                    vals = []
                    for b in new[key][:, s]:
                        if int(b) == ((I_END & 0xFFFFFFFF) if key == "PL" else F_END):
                            break
                        vals.append(vt.fmt_int(np.uint32(b).view(np.int32)) if key == "PL" else vt.fmt_float_bits(b))
                    field = ",".join(vals) or "."
                parts.append(field)
            new_cols.append(":".join(parts))
        out.append("\t".join(fixed + new_cols) + "\n")
        res.records += 1
    res.out = "".join(out)
    return res


def read_output(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


# ---- the generator ------------------------------------------------------------------------------------------------------------------
ALLELE_POOL = ["A", "C", "G", "T", "AT", "CG", "GA", "TTC", "<*>", "<NON_REF>", "N", "a"]
TAG_SETS = ("", "GL", "GL:PL", "GL:PL:GP")
# PL of a record drawn wide, by the record's index mod 3: the new values (less their minimum) end on either side of 127 / 128 and
# 32767 / 32768, so a file holds records of every width of htslib's integer writer; the last class also has values below -120 and -32760
PL_EDGES = [[0, 0, 1, 126, 127], [0, 0, 128, 129, 255, 32766, 32767], [0, 0, 32768, 70000, -70000, -121, -32761]]
PL_ODD = ["+00000000012", "00000000000", "-00000000001", " 7"]


def make_records(n_samples, n_records, seed, first_pos=1, n_old=None, n_new=None, tags="GL:PL:GP", qs=True, odd_share=0.0, wide_pl=False):
    """records as dicts: pos, alleles, target, info, keys, cols [sample] -> {key: text or None for a column cut short before it}.
    FORMAT is DP, the tags with an untouched field between them, AD last.  A sample is whole, ragged (GL and GP only: a ragged PL stops
    the run), '.' per field, all '.', a bare '.' column, or cut short; a record drawn odd has one sample with tokens outside the device
    grammar in GL and PL.  wide_pl draws PL from PL_EDGES, else 0 .. 255."""
    rng = np.random.default_rng(seed)
    pool = [ff._plain_token(rng) for _ in range(600)]
    gp_pool = ["%.6g" % x for x in rng.random(300)] + ["0", "1", "0.5", "1e-5", "2.5e-7"]
    N = n_samples
    keys = ["DP"]
    for j, t in enumerate([t for t in tags.split(":") if t]):
        keys += (["XS"] if j == 1 else []) + [t]
    keys.append("AD")
    recs = []
    for i in range(n_records):
        no = int(n_old or rng.integers(2, 6))
        alleles = [ALLELE_POOL[int(j)] for j in rng.choice(len(ALLELE_POOL), size=no, replace=False)]
        nn = int(n_new or rng.integers(2, no + 1))
        target = [alleles[int(j)] for j in rng.permutation(no)[:nn]]
        nG = no * (no + 1) // 2
        odd = int(rng.integers(0, N)) if rng.random() < odd_share else -1
        shapes = rng.integers(0, 14, size=N).tolist()
        u = rng.random((N, 3, nG)).tolist()
        idx = rng.integers(0, 600, size=(N, 3, nG)).tolist()
        cnt = rng.integers(1, nG + 1, size=N).tolist()
        keep = rng.integers(1, len(keys), size=N).tolist()
        dp = rng.integers(0, 100, size=N).tolist()
        cols = []
        for s in range(N):
            sh = 99 if s == odd else shapes[s]
            c = {}
            for key in keys:
                f = TAGS.index(key) if key in TAGS else -1
                n = cnt[s] if sh == 0 and key != "PL" else nG
                if key == "DP":
                    c[key] = str(dp[s])
                elif key == "XS":
                    c[key] = "x%d" % (dp[s] % 7)
                elif key == "AD":
                    c[key] = ",".join(str((dp[s] + a) % 9) for a in range(no))
                elif sh == 1:
                    c[key] = "."
                elif sh == 2:
                    c[key] = ",".join(["."] * nG)
                elif s == odd and key == "GL":
                    c[key] = ",".join(ff.ODD_TOKENS[j % len(ff.ODD_TOKENS)] for j in idx[s][f])
                elif s == odd and key == "PL":
                    c[key] = ",".join(PL_ODD[j % len(PL_ODD)] for j in idx[s][f])
                elif key == "GL":
                    c[key] = ",".join("." if x < 0.02 else "-inf" if x < 0.06 else "nan" if x < 0.08 else pool[j] for x, j in zip(u[s][f][:n], idx[s][f]))
                elif key == "PL":
                    c[key] = ",".join("." if x < 0.01 else str(PL_EDGES[i % 3][j % len(PL_EDGES[i % 3])] if wide_pl else j % 256) for x, j in zip(u[s][f], idx[s][f]))
                else:
                    c[key] = ",".join("." if x < 0.02 else "nan" if x < 0.03 else gp_pool[j % len(gp_pool)] for x, j in zip(u[s][f][:n], idx[s][f]))
            if sh == 3:                                      # a bare '.' column
                c = {k: ("." if k == "DP" else None) for k in keys}
            elif sh == 4:                                    # the column cut short behind a field (never to nothing)
                for key in keys[keep[s]:]:
                    c[key] = None
            cols.append(c)
        info = "DP=%d" % sum(dp) + (";QS=" + ",".join("%.6g" % x for x in rng.random(no)) if qs else "") + ";XI=0.50"
        recs.append(dict(pos=first_pos + i, alleles=alleles, target=target, info=info, keys=keys, cols=cols))
    return recs


def vcf_text(recs, n_samples):
    head = ['##fileformat=VCFv4.2', '##FILTER=<ID=PASS,Description="All filters passed">', '##contig=<ID=chr22,length=2147483647>',
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth">', '##INFO=<ID=QS,Number=R,Type=Float,Description="QS">',
            '##INFO=<ID=XI,Number=1,Type=Float,Description="An untouched value">',
            '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth">', '##FORMAT=<ID=XS,Number=1,Type=String,Description="An untouched field">',
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Allele depths">',
            '##FORMAT=<ID=GL,Number=G,Type=Float,Description="GL">', '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="PL">',
            '##FORMAT=<ID=GP,Number=G,Type=Float,Description="GP">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % s for s in range(n_samples))]
    out = head
    for r in recs:
        cols = [":".join(c[k] for k in r["keys"] if c[k] is not None) for c in r["cols"]]
        out.append("\t".join(["chr22", str(r["pos"]), "id%d" % r["pos"], r["alleles"][0], ",".join(r["alleles"][1:]) or ".", "30", "PASS", r["info"],
                              ":".join(r["keys"])] + cols))
    return "\n".join(out) + "\n"


def tsv_text(recs):
    return "".join(r["target"][0] + "\t" + ",".join(r["target"][1:]) + "\n" for r in recs)


def write_file(path, text, container):
    data = text.encode()
    if container == "gz":
        data = gzip.compress(data, 6)
    elif container == "bgz":
        data = ff.bgzf(data)
    else:
        assert container == "vcf"
    with open(path, "wb") as f:
        f.write(data)


# ---- BCF ------------------------------------------------------------------------------------------------------------------------------
# Records are the dicts bcf_reader.Reader.records() yields (floats as bits, integers with None for missing and "END"); `encode_bcf`
# writes such records the way htslib does (typed values, the narrowest integer type only where the model chooses one), so a generated
# input, the model's expected output and the program's output can be compared both decoded and as bytes.
BCF_DICT = {"PASS": 0, "DP": 1, "QS": 2, "XI": 3, "END": 4, "XS": 5, "AD": 6, "GL": 7, "PL": 8, "GP": 9}
_INT_FMT = {1: "<b", 2: "<h", 3: "<i"}
_INT_MISS = {1: -128, 2: -32768, 3: -2 ** 31}


def bcf_header_bytes(n_samples):
    lines = ['##fileformat=VCFv4.2', '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>', '##contig=<ID=chr22,length=2147483647,IDX=0>',
             '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth",IDX=1>', '##INFO=<ID=QS,Number=R,Type=Float,Description="QS",IDX=2>',
             '##INFO=<ID=XI,Number=1,Type=Float,Description="An untouched value",IDX=3>', '##INFO=<ID=END,Number=1,Type=Integer,Description="End",IDX=4>',
             '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth",IDX=1>', '##FORMAT=<ID=XS,Number=1,Type=Integer,Description="An untouched field",IDX=5>',
             '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Allele depths",IDX=6>', '##FORMAT=<ID=GL,Number=G,Type=Float,Description="GL",IDX=7>',
             '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="PL",IDX=8>', '##FORMAT=<ID=GP,Number=G,Type=Float,Description="GP",IDX=9>',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + "".join("\t" + c for c in (["FORMAT"] + ["ind%d" % s for s in range(n_samples)] if n_samples else []))]
    text = ("\n".join(lines) + "\n").encode() + b"\x00"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


def int_type(vals):
    """htslib's narrowing over the values that are neither missing nor end-of-vector"""
    real = [v for v in vals if v is not None and v != "END"]
    mn, mx = (min(real), max(real)) if real else (2 ** 31 - 1, -2 ** 31 + 1)
    return 1 if mx <= 127 and mn >= -120 else 2 if mx <= 32767 and mn >= -32760 else 3


def _tl(n, t):
    if n < 15:
        return bytes([(n << 4) | t])
    return bytes([0xF0 | t]) + (bytes([0x11, n]) if n < 128 else b"\x12" + struct.pack("<H", n))


def _ints(vals, t):
    return b"".join(struct.pack(_INT_FMT[t], _INT_MISS[t] if v is None else _INT_MISS[t] + 1 if v == "END" else v) for v in vals)


def _tstr(s):
    b = s.encode()
    return _tl(len(b), 7) + b


def encode_record(r, n_samples):
    sh = struct.pack("<iiiIII", 0, r["pos0"], r["rlen"], r["qual"], (len(r["alleles"]) << 16) | len(r["info"]), (len(r["fmt"]) << 24) | n_samples)
    sh += _tstr("" if r["id"] == "." else r["id"]) + b"".join(_tstr(a) for a in r["alleles"])
    filt = [BCF_DICT[f] for f in r["filter"]]
    sh += (_tl(len(filt), 1) + _ints(filt, 1)) if filt else b"\x00"
    for k, t, v in r["info"]:
        sh += bytes([0x11, BCF_DICT[k]])
        sh += b"\x00" if t == 0 else _tl(len(v), 5) + struct.pack("<%dI" % len(v), *v) if t == 5 else _tstr(v) if t == 7 else _tl(len(v), t) + _ints(v, t)
    ind = b""
    for k, t, per in r["fmt"]:
        n = len(per[0])
        ind += bytes([0x11, BCF_DICT[k]]) + _tl(n, t)
        ind += b"".join(struct.pack("<%dI" % n, *v) for v in per) if t == 5 else b"".join(_ints(v, t) for v in per)
    return struct.pack("<II", len(sh), len(ind)) + sh + ind


def encode_bcf(recs, n_samples):
    return bcf_header_bytes(n_samples) + b"".join(encode_record(r, n_samples) for r in recs)


def bcf_records(recs, n_samples, end_every=0):
    """the generator's records (make_records) as BCF records: a token is the value htslib reads from it, a field '.' or cut short is the
    missing value and the end-of-vector fill, the vector length is the record's largest count, integers at the narrowest type that holds
    the record's values; XS becomes an integer.  end_every: every such record carries INFO/END (and an rlen that follows it)."""
    out = []
    for i, r in enumerate(recs):
        info = []
        for kv in r["info"].split(";"):
            k, v = kv.split("=")
            if k == "QS":
                info.append((k, 5, [float_value(x) for x in v.split(",")]))
            elif k == "XI":
                info.append((k, 5, [float_value(v)]))
            else:
                info.append((k, int_type([int(v)]), [int(v)]))
        rlen = len(r["alleles"][0])
        if end_every and i % end_every == 0:
            info.append(("END", 2, [r["pos"] + 40]))
            rlen = 41
        fmt = []
        for key in r["keys"]:
            toks = [["."] if c[key] is None else c[key].split(",") for c in r["cols"]]
            n = max(len(t) for t in toks)
            if key in ("GL", "GP"):
                fmt.append((key, 5, [[float_value(x) for x in t] + [F_END] * (n - len(t)) for t in toks]))
                continue
            per = [[None if x == "." else int(x.lstrip("x")) for x in t] + ["END"] * (n - len(t)) for t in toks]
            fmt.append((key, int_type([x for v in per for x in v]), per))
        out.append(dict(chrom="chr22", pos0=r["pos"] - 1, rlen=rlen, qual=int(np.float32(30).view(np.uint32)), id="id%d" % r["pos"], alleles=list(r["alleles"]),
                        filter=["PASS"], info=info, fmt=fmt))
    return out


def _bits_of(per, nGo, pl):
    a = np.empty((nGo, len(per)), np.uint32)
    for s, v in enumerate(per):
        for g in range(nGo):
            x = (I_END if pl else F_END) if g >= len(v) else v[g]
            if pl:
                x = I_MISSING if x is None else I_END if x == "END" else x
            a[g, s] = x & 0xFFFFFFFF
    return a


class BcfResult:
    def __init__(self):
        self.records, self.stop = [], None

    @property
    def returncode(self):
        return 1 if self.stop else 0


def run_bcf(recs, targets):
    """the run of setalleles_hip on BCF records (dicts as bcf_reader yields them) -> the records it writes.  The stops of the header pass
    (alleles, lacks, qs, many, count) leave no record; a PL overflow ("pl") leaves the records before it"""
    res = BcfResult()
    for i, r in enumerate(recs[:len(targets)]):
        pos, nGo = r["pos0"] + 1, sm.n_gt(len(r["alleles"]))
        if len(r["alleles"]) > 5:
            res.stop = ("alleles", pos)
        elif any(a not in r["alleles"] for a in targets[i]):
            res.stop = ("lacks", pos)
        elif any(k == "QS" and len(v) != len(r["alleles"]) for k, t, v in r["info"]):
            res.stop = ("qs", pos)
        else:
            seen = set()
            for k, t, per in r["fmt"]:
                if k in TAGS and k not in seen and len(per[0]) > 0:
                    seen.add(k)
                    if len(per[0]) > nGo:
                        res.stop = ("many", pos)
        if res.stop:
            return res
    if len(recs) != len(targets):
        res.stop = ("count", None)
        return res
    for r, tgt in zip(recs, targets):
        o2n = sm.allele_map(r["alleles"], tgt)
        g2g = sm.genotype_map(o2n)
        nGo, nGn = sm.n_gt(len(r["alleles"])), sm.n_gt(len(tgt))
        new = dict(r, alleles=list(tgt), rlen=r["rlen"] if any(k == "END" for k, _, _ in r["info"]) else len(tgt[0]))
        new["info"] = [(k, t, [v[r["alleles"].index(a)] for a in tgt]) if k == "QS" else (k, t, v) for k, t, v in r["info"]]
        fmt, seen = [], set()
        for k, t, per in r["fmt"]:
            if k not in TAGS or k in seen or len(per[0]) == 0:
                fmt.append((k, t, per))
                continue
            seen.add(k)
            g = sm.scatter(_bits_of(per, nGo, k == "PL"), g2g, nGn, 0)
            if k != "PL":
                fmt.append((k, 5, [[int(x) for x in col] for col in norm_float(g, k == "GP").T]))
                continue
            out, over = norm_pl(g)
            if over:
                res.stop = ("pl", r["pos0"] + 1)
                return res
            per2 = [[None if x == I_MISSING else "END" if x == I_END else int(x) for x in col] for col in out.view(np.int32).T]
            fmt.append((k, int_type([x for v in per2 for x in v]), per2))
        new["fmt"] = fmt
        res.records.append(new)
    return res


def write_bcf(path, recs, n_samples, container):
    data = encode_bcf(recs, n_samples)
    with open(path, "wb") as f:
        f.write(ff.bgzf(data) if container == "bcf.gz" else data)


def read_bcf(path):
    """(the decompressed bytes behind the header, the decoded records) of a BCF file, raw or BGZF"""
    rd = bcf_reader.Reader(path)
    return rd.raw[rd.off:], list(rd.records())
