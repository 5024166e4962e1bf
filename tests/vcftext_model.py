"""Plain Python model of the VCF text the host writer appends behind a simulated record's eight fixed columns (host/vcf_sink.h,
Sink::encode_rec, text branch) and of the number formatter it uses (host/host_util.h put_float / put_int, htslib's kputd):

    "\\t" KEYS ( "\\t" sample_0 ) ... ( "\\t" sample_{N-1} ) "\\n"

Floats: the missing pattern -> ".", NaN -> "nan", +-0 -> "0" / "-0", the sign first; [1e-4, 999999] in kputd's integer form
(int(d * 1e10) in double arithmetic plus half a unit of the 6th significant digit), otherwise Python's '%g' (correctly rounded from the
exact binary value, ties to even: glibc's %g)."""
import struct

import numpy as np

FLOAT_MISSING_BITS = 0x7F800001
INT32_MISSING = -(2 ** 31)
ONE, PER_G, PER_A = 0, 1, 2
_ADD = [(0.001, 5), (0.01, 50), (0.1, 500), (1, 5000), (10, 50000), (100, 500000), (1000, 5000000), (10000, 50000000), (100000, 500000000)]


def fmt_float_bits(b):
    b = int(b) & 0xFFFFFFFF
    if b == FLOAT_MISSING_BITS:
        return "."
    d = struct.unpack("<f", struct.pack("<I", b))[0]
    if d != d:
        return "nan"
    if d == 0:
        return "-0" if b >> 31 else "0"
    sign = ""
    if d < 0:
        sign, d = "-", -d
    if not (0.0001 <= d <= 999999):
        return sign + ("%g" % d)
    i = int(d * 10000000000.0)
    for lim, add in _ADD:
        if d < lim:
            i += add
            break
    else:
        i += 5000000000
    dig = str(i)
    n = len(dig)
    if n <= 10:
        out = "0." + "0" * (10 - n) + dig[:min(n, 6)]
    else:
        ip = n - 10
        out = dig[:ip] + ("." + dig[ip:6] if ip < 6 else "")
    if "." in out:
        out = out.rstrip("0").rstrip(".")
    return sign + out


def fmt_int(v):
    v = int(v)
    return "." if v == INT32_MISSING else "%d" % v


def n_values(kind, nA):
    return 1 if kind == ONE else nA * (nA + 1) // 2 if kind == PER_G else nA


def render(fields, site_status, n_alleles, n_samples):
    """(bytes, offsets) of a tile: fields = [(key, numpy [n_sites, stride] int32 / float32, ONE / PER_G / PER_A)], sample-major slabs"""
    keys = ":".join(k for k, _, _ in fields) or "."
    cache = []
    for _, a, _ in fields:                                         # every distinct value formatted once
        if a.dtype == np.float32:
            u = np.unique(a.view(np.uint32))
            cache.append({int(x): fmt_float_bits(x) for x in u})
        else:
            u = np.unique(a)
            cache.append({int(x): fmt_int(x) for x in u})
    parts, offsets, pos = [], [0], 0
    for i in range(len(site_status)):
        if site_status[i] < 0:
            offsets.append(pos)
            continue
        nA = int(n_alleles[i])
        cols = []
        for f, (_, a, kind) in enumerate(fields):
            n = n_values(kind, nA)
            v = a[i].view(np.uint32) if a.dtype == np.float32 else a[i]
            v = v[: n_samples * n].reshape(n_samples, n)
            c = cache[f]
            cols.append([",".join(c[int(x)] for x in row) for row in v])
        if fields:
            text = "\t" + keys + "".join("\t" + ":".join(col[s] for col in cols) for s in range(n_samples)) + "\n"
        else:
            text = "\t." + "\t." * n_samples + "\n"
        b = text.encode()
        parts.append(b)
        pos += len(b)
        offsets.append(pos)
    return b"".join(parts), np.array(offsets, dtype=np.int64)


def _f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def float_corpus(n_random=60000, seed=1):
    """bit patterns of every class boundary of the formatter, plus random patterns"""
    pats = {0, 0x80000000, FLOAT_MISSING_BITS, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800002, 0x7FFFFFFF, 0xFFFFFFFF,
            1, 2, 3, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFF, 0x80000001, 0x807FFFFF, 0x80800000}
    for v in (1e-4, 999999.0, 9.999995, 99999.95, 0.99999949, 0.000099999, 999999.5, 1e6, 1e-5, 1e5, 1.0, 10.0, 0.1, 0.001, 0.01, 100.0, 1000.0,
              10000.0, 123456.5, 1e38, 1e-38, 9.999995e-5, 9.999995e5, 1234565.0, 1234575.0, 2.5e-45, 3.4e38, 0.5, 99999.95, 999.9995,
              1e-10, 1e-20, 1e-30, 1e-40, 1e7, 1e10, 1e20, 1e30):
        b = _f32(v)
        for d in range(-8, 9):
            for sgn in (0, 0x80000000):
                pats.add(((b + d) & 0x7FFFFFFF) | sgn)
    for x in range(1000000, 1000000 + 4000, 1):                 # integer-valued floats above 1e6: ties of the 6th digit
        pats.add(_f32(float(x * 5 + 5)))
    for x in (1234565, 1234575, 2000005, 9999995, 9999985, 10000005, 12345650, 99999950):
        pats.add(_f32(float(x)))
    for e10 in range(-45, 39):                                   # decade boundaries: 10^k and 9.999995 x 10^k, a few ulps each side
        for m in (1.0, 9.999995, 9.9999949, 9.9999951, 5.0, 1.000005):
            try:
                b = _f32(m * 10.0 ** e10)
            except OverflowError:
                continue
            for d in range(-3, 4):
                pats.add((b + d) & 0x7FFFFFFF)
    rng = np.random.default_rng(seed)
    pats.update(int(x) for x in rng.integers(0, 2 ** 32, size=n_random, dtype=np.uint64))
    pats.update(int(x) for x in (rng.integers(0x38000000, 0x49800000, size=n_random // 2, dtype=np.uint64)))   # 3e-5 .. 1e6
    return np.array(sorted(pats), dtype=np.uint32)
