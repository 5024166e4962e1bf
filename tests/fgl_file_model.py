"""Plain Python model of fetchgl_hip (vcfgl_amd/csrc/misc: the reference's misc/fetchGl on a record file) and a generator of record
files for it.  The model builds on fetchgl_model (genotype_index, fmt_value_bits) and, for BCF, on bcf_reader.

Rules (vcfgl_amd/csrc/misc/fgl_core.h):
    GL first       a header without FORMAT/GL (a BCF: not Type=Float), or a record whose FORMAT lacks GL, stops the run at that record
    genotype       allele j matches a character when the first character of its name equals it, the last match wins,
                   g = hi (hi + 1) / 2 + lo; a record that lacks either allele has a message and no line
    values         a sample column that ends before the GL field, or whose field is '.', is one missing value; n_gls is the largest
                   value count of the record (a BCF: the vector length); g < c the value, c <= g < n_gls END, '.' MISSING
    stops          a column count other than the header's sample count, g >= n_gls, a picked token strtod does not take whole
    a text value   the nearest double of the token, then the nearest float of that; printed as %f / inf / -inf / nan / -nan
`in_grammar` is the device grammar: a record with a picked token outside it is redone on the host (`Result.redone` counts them).

The generator (`make_records`, `write_file`) gives VCF text, gzip, BGZF and BCF (the tests' own encoder: bcfin_cases) with 1 to 5
alleles, GL at every place of FORMAT, short columns, '.' fields, ragged counts, infinities and NaN, values of 1 to 15 digits with
exponents and a leading '+', and an `odd_share` of records that hold tokens outside the device grammar."""
import functools
import gzip
import re
import struct
import zlib

import numpy as np

import bcf_reader
import bcfin_cases as bc
import fetchgl_model as fm

MSG_SKIP = "Requested genotype %s not found at position %d. Skipping...\n"
MSG_FOUND = "Requested genotype's first allele corresponds to allele %d and second allele corresponds to allele %d at position %d.\n"
LETTERS = "ACGT<"
FIXED_ALLELES = ["A", "C", "G", "T", "<*>"]
GENOTYPES = [LETTERS[lo] + LETTERS[hi] for hi in range(5) for lo in range(hi + 1)]      # g = 0 .. 14 on FIXED_ALLELES
FORMATS = ["GL", "GT:GL", "GL:GT", "GT:DP:GL", "GT:GL:DP", "GL:DP:GT", "DP:GL"]
CONTAINERS = ("vcf", "gz", "bgz", "bcf")

_TOKEN = re.compile(r"[+-]?([0-9]+)?(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]{1,3}))?\Z")
_HEX = re.compile(r"[+-]?0[xX]")


def in_grammar(tok):
    """the device grammar of fgl_core.h"""
    if tok in (".", "inf", "-inf", "nan"):
        return True
    m = _TOKEN.match(tok)
    if not m or not ((m.group(1) or "") + (m.group(2) or "")):
        return False
    ip, fr, ex = m.group(1) or "", m.group(2) or "", int(m.group(3) or 0)
    sig = len((ip + fr).lstrip("0"))
    return sig <= 15 and abs(ex - len(fr)) <= 22


@functools.lru_cache(maxsize=None)
def token_bits(tok):
    """the float32 bits htslib reads for a token that is not '.'; None: strtod does not take it whole"""
    try:
        d = float.fromhex(tok) if _HEX.match(tok) else float(tok)
    except (ValueError, OverflowError):
        return None
    if tok != tok.strip() or "_" in tok:
        return None
    with np.errstate(over="ignore"):
        bits = int(np.array([d], np.float64).astype(np.float32).view(np.uint32)[0])
    if d != d:
        bits = 0xFFC00000 if tok.lstrip().startswith("-") else 0x7FC00000
    return bits


def value_text(bits):
    return fm.fmt_value_bits(bits, fm.FLOAT)


class Result:
    def __init__(self):
        self.stdout, self.messages = [], []
        self.stop = None                   # (kind, POS): "gl", "columns", "range", "token"
        self.redone = 0                    # records with a line whose picked tokens leave the device grammar
        self.lines = 0

    @property
    def returncode(self):
        return 1 if self.stop else 0


def _record(res, pos, first_chars, gt, picked):
    """picked(g) -> list of value strings, or raises Stop"""
    j = [-1, -1]
    for i, c in enumerate(first_chars):
        for k in range(2):
            if c == gt[k]:
                j[k] = i
    if min(j) < 0:
        res.messages.append(MSG_SKIP % (gt, pos))
        return True
    res.messages.append(MSG_FOUND % (j[0], j[1], pos))
    g = max(j) * (max(j) + 1) // 2 + min(j)
    vals = picked(g)
    if vals is None:
        return False
    res.stdout.append("%d," % pos + ",".join(vals) + "\n")
    res.lines += 1
    return True


def run_text(text, gt):
    """the run of fetchgl_hip on VCF text"""
    res = Result()
    header = [ln for ln in text.split("\n") if ln.startswith("##")]
    names = [ln for ln in text.split("\n") if ln.startswith("#CHROM")]
    N = len(names[0].split("\t")) - 9 if names else 0
    defined = any(h.startswith("##FORMAT=<ID=GL,") for h in header)
    for ln in text.split("\n"):
        if not ln or ln[0] == "#":
            continue
        f = ln.split("\t")
        pos = int(f[1])
        keys = f[8].split(":")
        if not defined or "GL" not in keys:
            res.stop = ("gl", pos)
            break
        k = keys.index("GL")
        alleles = [f[3]] + ([] if f[4] == "." else f[4].split(","))

        def picked(g, f=f, k=k, pos=pos):
            cols = f[9:]
            fields = []
            for col in cols:
                sub = col.split(":")
                fields.append(sub[k].split(",") if k < len(sub) else ["."])
            if any(g < len(t) and not in_grammar(t[g]) for t in fields[:N]):
                res.redone += 1
            if len(cols) != N:
                res.stop = ("columns", pos)
                return None
            if g >= max(len(t) for t in fields):
                res.stop = ("range", pos)
                return None
            vals = []
            for t in fields:
                if g >= len(t):
                    vals.append("END")
                elif t[g] == ".":
                    vals.append("MISSING")
                else:
                    b = token_bits(t[g])
                    if b is None:
                        res.stop = ("token", pos)
                        return None
                    vals.append(value_text(b))
            return vals

        if not _record(res, pos, [a[:1] for a in alleles], gt, picked):
            break
    return res


def run_bcf(path, gt):
    """the run of fetchgl_hip on a BCF file"""
    res = Result()
    rd = bcf_reader.Reader(path)
    defined = rd.fmt_type.get("GL") == "Float"
    for r in rd.records():
        pos = r["pos0"] + 1
        gl = [(t, per) for k, t, per in r["fmt"] if k == "GL"]
        if not defined or not gl or gl[0][0] != 5:
            res.stop = ("gl", pos)
            break
        per = gl[0][1]

        def picked(g, per=per, pos=pos):
            if g >= len(per[0]):
                res.stop = ("range", pos)
                return None
            return [value_text(v[g]) for v in per]

        if not _record(res, pos, [a[:1] for a in r["alleles"]], gt, picked):
            break
    return res


def run_file(path, gt):
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return run_bcf(path, gt) if raw[:3] == b"BCF" else run_text(raw.decode(), gt)


# ---- the generator ------------------------------------------------------------------------------------------------------------------
ALLELE_POOL = ["A", "C", "G", "T", "AT", "CG", "GA", "TTC", "<*>", "<NON_REF>", "N", "a"]
ODD_TOKENS = ["1234567890.123456", "-0.1234567890123456", "1e-30", "-1.5e25", "12345e-28", "INF", "-Infinity", "1e400", "-1e-400", "0x1.8p1", "-0X1P-3",
              "1e0005"]


def _plain_token(rng):
    """a token inside the device grammar: 1 to 15 digits, a point anywhere, an exponent, a leading '+'"""
    n = int(rng.integers(1, 16))
    digits = "".join(str(int(d)) for d in rng.integers(0, 10, size=n))
    cut = int(rng.integers(0, n + 1))
    style = int(rng.integers(0, 6))
    if style == 0:                                      # a GL as the writers print it
        return "-%.6g" % float(np.exp(rng.uniform(np.log(1e-4), np.log(5000.0))))
    tok = digits[:cut] + ("." + digits[cut:] if cut < n or style == 1 else "")
    if tok.startswith("."):
        tok = ("0" if style == 2 else "") + tok
    behind = n - cut
    if style >= 3:
        lo, hi = -22 + behind, 22 + behind
        ex = int(rng.integers(max(lo, -30), min(hi, 30) + 1))
        tok += ("e", "E")[style & 1] + ("%+d" % ex if style == 5 else str(ex))
    return ("-", "", "+", "-")[int(rng.integers(0, 4))] + tok


def make_records(n_samples, n_records, seed, first_pos=1, odd_share=0.0, fixed_alleles=False, fmt=None):
    """records as dicts: pos, alleles, keys (FORMAT), cols [sample] -> {key: text or None for a column cut short before it}.
    Every record has one sample with the full count of values (no genotype of its alleles is out of range); a record drawn odd has a
    sample whose every GL value is a token outside the device grammar.  (The draws of a record are made for all its samples at once,
    from a pool of 600 plain tokens per file: a file of 257 samples is made in a second.)"""
    rng = np.random.default_rng(seed)
    pool = [_plain_token(rng) for _ in range(600)]
    N = n_samples
    recs = []
    for i in range(n_records):
        if fixed_alleles:
            alleles = list(FIXED_ALLELES)
        else:
            alleles = [ALLELE_POOL[int(j)] for j in rng.choice(len(ALLELE_POOL), size=int(rng.integers(1, 6)), replace=False)]
            if alleles[0].startswith("<"):
                alleles[0] = "G"
        nG = len(alleles) * (len(alleles) + 1) // 2
        keys = (fmt or FORMATS[int(rng.integers(0, len(FORMATS)))]).split(":")
        full = int(rng.integers(0, N))
        odd = int(rng.integers(0, N)) if rng.random() < odd_share else -1
        shapes = rng.integers(0, 12, size=N)
        shapes[full] = 99
        if odd >= 0:
            shapes[odd] = 99
        counts = np.where(shapes > 2, nG, rng.integers(1, nG + 1, size=N)).tolist()
        u = rng.random((N, nG)).tolist()
        idx = rng.integers(0, len(pool), size=(N, nG)).tolist()
        gt = rng.integers(-1, len(alleles), size=(N, 2)).tolist()
        ph = rng.integers(0, 2, size=N).tolist()
        dp_u, dp = rng.random(N).tolist(), rng.integers(0, 100, size=N).tolist()
        keep = rng.integers(1, max(len(keys), 2), size=N).tolist()
        shapes = shapes.tolist()
        cols = []
        for s in range(N):
            c = {}
            for key in keys:
                if key == "GT":
                    a, b = gt[s]
                    c[key] = ("." if a < 0 else str(a)) + "/|"[ph[s]] + ("." if b < 0 else str(b))
                elif key == "DP":
                    c[key] = "." if dp_u[s] < 0.1 else str(dp[s])
                elif s == odd:
                    c[key] = ",".join(ODD_TOKENS[j % len(ODD_TOKENS)] for j in idx[s])
                elif shapes[s] == 3:
                    c[key] = "."
                else:
                    c[key] = ",".join("." if x < 0.05 else "-inf" if x < 0.10 else "inf" if x < 0.12 else "nan" if x < 0.14 else pool[j]
                                      for x, j in zip(u[s][:counts[s]], idx[s]))
            if shapes[s] == 4:                             # the column cut short behind a field (never to nothing)
                for key in keys[keep[s]:]:
                    c[key] = None
            cols.append(c)
        recs.append(dict(pos=first_pos + i, alleles=alleles, keys=keys, cols=cols))
    return recs


def vcf_text(recs, n_samples, define_gl=True):
    head = ['##fileformat=VCFv4.2', '##FILTER=<ID=PASS,Description="All filters passed">', '##contig=<ID=chr22,length=2147483647>',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth">',
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="PL">']
    if define_gl:
        head.append('##FORMAT=<ID=GL,Number=G,Type=Float,Description="GL">')
    head.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % s for s in range(n_samples)))
    out = head
    for r in recs:
        cols = [":".join(c[k] for k in r["keys"] if c[k] is not None) for c in r["cols"]]
        out.append("\t".join(["chr22", str(r["pos"]), ".", r["alleles"][0], ",".join(r["alleles"][1:]) or ".", ".", "PASS", ".", ":".join(r["keys"])] + cols))
    return "\n".join(out) + "\n"


def bgzf(data, block=60000):
    out = b""
    for at in list(range(0, len(data), block)) + [len(data)]:               # (the last member is the empty end-of-file block)
        chunk = data[at:at + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(chunk) + z.flush()
        out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out


def _typed_len(n, t):
    return bytes([(n << 4) | t]) if n < 15 else bytes([0xF0 | t, 0x11, n])


def bcf_bytes(recs, n_samples, gl_type="Float"):
    """the BCF of the records: the stored float of a token is what htslib reads from the text; a field cut short or '.' is the missing
    value and the end-of-vector fill, and the vector length is the record's largest count.  (A token strtod refuses cannot be stored.)"""
    GT, DP, GL = 1, 2, 4
    out = [bc.bcf_header([b"ind%d" % s for s in range(n_samples)], length=2147483647,
                         extra=[b'##FORMAT=<ID=GL,Number=G,Type=%s,Description="GL",IDX=4>' % gl_type.encode()])]
    for r in recs:
        fields = []
        for key in r["keys"]:
            if key == "GT":
                data = b""
                for c in r["cols"]:
                    t = c[key]
                    if t is None:
                        data += bytes([0, 0x81])
                        continue
                    a, b = re.split(r"[/|]", t)
                    ph = 1 if "|" in t else 0
                    data += bytes([bc.gt_value(-1 if a == "." else int(a)), bc.gt_value(-1 if b == "." else int(b), ph)])
                fields.append((GT, 1, 2, data))
            elif key == "DP":
                fields.append((DP, 1, 1, b"".join(bytes([0x80]) if c[key] in (None, ".") else bytes([int(c[key])]) for c in r["cols"])))
            else:
                toks = [["."] if c[key] is None else c[key].split(",") for c in r["cols"]]
                n = max(len(t) for t in toks)
                data = b""
                for t in toks:
                    bits = [fm.MISSING_BITS if x == "." else token_bits(x) for x in t] + [fm.END_BITS] * (n - len(t))
                    data += struct.pack("<%dI" % n, *bits)
                fields.append((GL, 5, n, data))
        shared = struct.pack("<iiiIII", 0, r["pos"] - 1, 1, 0x7F800001, (len(r["alleles"]) << 16) | 0, (len(fields) << 24) | n_samples)
        shared += bc.typed_str(b".") + b"".join(bc.typed_str(a.encode()) for a in r["alleles"]) + bytes([0x11, 0x00])
        indiv = b"".join(bytes([0x11, key]) + _typed_len(n, t) + data for key, t, n, data in fields)
        out.append(struct.pack("<II", len(shared), len(indiv)) + shared + indiv)
    return b"".join(out)


def write_file(path, recs, n_samples, container, **kw):
    """container: 'vcf', 'gz' (gzip), 'bgz' (BGZF) or 'bcf' (raw BCF)"""
    if container == "bcf":
        data = bcf_bytes(recs, n_samples, **kw)
    else:
        data = vcf_text(recs, n_samples, **kw).encode()
        if container == "gz":
            data = gzip.compress(data)
        elif container == "bgz":
            data = bgzf(data)
    with open(path, "wb") as f:
        f.write(data)
    return path
