"""Plain Python model of the reference's misc/fetchGl: per record of a VCF, the FORMAT/GL value of one requested genotype for every
sample, "POS,gl_0,...,gl_{N-1}".

    allele j matches a character of the genotype string when the first character of its name equals it (the last match wins);
    a record that lacks one of the two alleles has no line; g = max (max + 1) / 2 + min
    a value is "MISSING" for "." and otherwise '%f' of the float htslib reads: the nearest double of the text, then the nearest float

`file_lines` works on VCF text; `fmt_value_bits` is the per-value function over float32 bit patterns for both value modes of the device
formatter (include/vcfgl_hip.h, VGL_FETCHGL_*), TEXT built on vcftext_model.fmt_float_bits; `render` applies it to a tile's arrays and
gives the (bytes, offsets) contract of vgl_fetchgl_format_device.  `exact_f` is %f by exact rational arithmetic: Python's own '%f' is
then not the only witness."""
import struct
from fractions import Fraction

import numpy as np

import vcftext_model

FLOAT, TEXT = 0, 1
MISSING_BITS, END_BITS = 0x7F800001, 0x7F800002
LETTERS = "ACGT<"


def _f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _val(b):
    return struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0]


def fmt_text_value(text):
    """what the tool prints for one value of a VCF text file"""
    if text == ".":
        return "MISSING"
    return "%f" % float(np.float32(float(text)))


def fmt_value_bits(b, mode):
    b = int(b) & 0xFFFFFFFF
    if b == MISSING_BITS:
        return "MISSING"
    v = _val(b)
    if mode == FLOAT:
        if b == END_BITS:
            return "END"
        if v != v:
            return "-nan" if b >> 31 else "nan"
        return "%f" % v
    if v == v and abs(v) >= 1e21 and abs(v) != float("inf"):
        return "%f" % v
    return fmt_text_value(vcftext_model.fmt_float_bits(b))


def exact_f(b):
    """%f of a finite float32 by exact arithmetic: six decimals, ties to even, the sign first"""
    b = int(b) & 0xFFFFFFFF
    x = Fraction(_val(b & 0x7FFFFFFF)) * 1000000
    n = x.numerator // x.denominator
    r = x - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return ("-" if b >> 31 else "") + "%d.%06d" % (n // 1000000, n % 1000000)


def genotype_index(names, gt):
    """names: the first characters of a record's alleles; None when the record lacks one of the two"""
    j = [-1, -1]
    for i, c in enumerate(names):
        for k in range(2):
            if c == gt[k]:
                j[k] = i
    if min(j) < 0:
        return None
    hi, lo = max(j), min(j)
    return hi * (hi + 1) // 2 + lo


def file_lines(vcf_text, gt):
    """the tool's stdout for the text of a VCF file"""
    out = []
    for ln in vcf_text.splitlines():
        if not ln or ln[0] == "#":
            continue
        f = ln.split("\t")
        alleles = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        g = genotype_index([a[0] for a in alleles], gt)
        if g is None:
            continue
        k = f[8].split(":").index("GL")
        vals = []
        for col in f[9:]:
            sub = col.split(":")
            gls = sub[k].split(",") if k < len(sub) else ["."]
            vals.append(fmt_text_value(gls[g]) if g < len(gls) else "END")
        out.append(f[1] + "," + ",".join(vals) + "\n")
    return "".join(out)


def render(site_status, n_alleles, a2b, gl_bits, layout, G, a, b, mode):
    """(bytes, offsets) of a tile: gl_bits uint32, planes [n_sites][G][N] (layout 0) or sample-major slabs [n_sites][G * N] (layout 1)"""
    n_sites = len(site_status)
    N = gl_bits.size // (n_sites * G) if n_sites else 0
    flat = gl_bits.reshape(n_sites, G * N)
    cache = {}
    parts, offsets, pos = [], [0], 0
    for i in range(n_sites):
        nA = min(max(int(n_alleles[i]), 0), 5)
        nG = nA * (nA + 1) // 2
        g = genotype_index([LETTERS[c] if 0 <= c <= 4 else "?" for c in a2b[i][:nA]], LETTERS[a] + LETTERS[b]) if site_status[i] >= 0 else None
        if g is None or nG > G:
            offsets.append(pos)
            continue
        row = flat[i][g * N:(g + 1) * N] if layout == 0 else flat[i][g:N * nG:nG]
        vals = []
        for x in row:
            x = int(x)
            if x not in cache:
                cache[x] = fmt_value_bits(x, mode)
            vals.append(cache[x])
        t = (",".join(vals) + "\n").encode()
        parts.append(t)
        pos += len(t)
        offsets.append(pos)
    return b"".join(parts), np.array(offsets, dtype=np.int64)


def lines(pos, text, offsets):
    """the CSV: "POS," in front of every non-empty site text"""
    out = []
    for i in range(len(offsets) - 1):
        if offsets[i + 1] > offsets[i]:
            out.append(b"%d," % int(pos[i]) + bytes(text[int(offsets[i]):int(offsets[i + 1])]))
    return b"".join(out)


def value_set(n_random=100000, seed=20):
    """float32 bit patterns: every exact tie of the sixth decimal +-k 2^-7 (odd k up to 2^12) and its neighbours, carries, zeros, the
    sentinels, NaNs, infinities, 6-digit GL-like values (|v| >= 16: where TEXT and FLOAT differ), both sides of 1e-4, 999999 and 1e21,
    the smallest denormal, FLT_MAX, and random patterns"""
    pats = {0, 0x80000000, MISSING_BITS, END_BITS, 0x7FC00000, 0xFFC00000, 0x7F800003, 0xFF800001, 0x7F800000, 0xFF800000, 1, 0x80000001,
            0x7F7FFFFF, 0xFF7FFFFF, 0x007FFFFF, 0x00800000}
    for k in range(1, 2 ** 12 + 1, 2):
        b = _f32(k / 128.0)
        for d in (-1, 0, 1):
            pats.add(b + d)
            pats.add((b + d) | 0x80000000)
    for v in (0.9999995, 9.9999995, 99.9999995, 0.0000005, 0.0000015, 4.7683716e-07, 9.5367432e-07, 1e-17, 1e-18, 1e-7, 1e-8, 4294967296.0,
              4294967040.0, 16777216.0, 16777215.0, 1e10, 1e15, 1e20, 1e22, 1e30):
        b = _f32(v)
        for d in range(-2, 3):
            pats.add(b + d)
            pats.add((b + d) | 0x80000000)
    for v in (1e-4, 999999.0, 1e21):
        b = _f32(v)
        for d in range(-4, 5):
            pats.add(b + d)
            pats.add((b + d) | 0x80000000)
    rng = np.random.default_rng(seed)
    for lo, hi in ((1e-6, 1e-3), (1e-3, 1.0), (1.0, 16.0), (16.0, 1000.0), (1000.0, 7000.0)):   # GL-like: -1e-6 .. -7000, 6 significant digits
        for v in np.exp(rng.uniform(np.log(lo), np.log(hi), size=400)):
            pats.add(_f32(-float("%.6g" % v)))
            pats.add(_f32(-float(v)))
    pats.update(_f32(v) for v in (-123.457, -8.26429, -7000.0, -1e-6, -0.000123457, -6999.99))
    pats.update(int(x) for x in rng.integers(0, 2 ** 32, size=n_random, dtype=np.uint64))
    return np.array(sorted(pats), dtype=np.uint32)
