"""Hand-built inputs of the BCF genotype decoder's tests: the record sets of the kernel and core tests (GT slices with the bytes that lie
between them in a file), the BCF file of odd records of the CLI tests, and a BCF writer for synthetic genotypes.  Each comes with the
records that were CONSTRUCTED to fall outside the plain rule; tests/test_bcfin_cpu.py checks that the model hands exactly those to the
host, so that a device path which hands everything back cannot pass the kernel tests."""
import functools
import struct

import numpy as np

import bcfin_model as bm

MAP_BINARY = [0, 1, -1, -1, -1]          # make_site's ra[] with --source 0
MAP_ACGT = [2, 3, 0, 1, 4]               # with --source 1: REF G, ALT T,A,C,<*>
FILL = 0xEE                              # the bytes between two slices (other FORMAT fields, the next record's shared block)


def gt_value(allele, phased=0):
    """the BCF value of an allele index (-1: the missing allele '.')"""
    return ((allele + 1) << 1) | phased


class Case:
    """records of one call: the bytes, per record (gt_begin, gt_type, gt_n, n_alleles, allele_map), n_samples, constructed fallbacks"""

    def __init__(self, n_samples):
        self.N, self.parts, self.size = n_samples, [], 0
        self.begin, self.type, self.n, self.nal, self.amap, self.fallback = [], [], [], [], [], set()

    def pad(self, k):
        self.parts.append(bytes([FILL]) * k); self.size += k
        return self

    def pad_to(self, residue, modulus=16):
        return self.pad((residue - self.size) % modulus)

    def add(self, vals=None, gt_type=1, nal=2, amap=MAP_BINARY, fallback=False, raw=None, n=None):
        """vals: N lists of n entries (integers, "E", "M") of an integer type; or raw bytes with n given (any type)"""
        if raw is None:
            n, w = len(vals[0]), bm.WIDTH[gt_type]
            assert len(vals) == self.N and all(len(v) == n for v in vals)
            raw = b"".join(bm.encode(x, w) for v in vals for x in v)
        if fallback:
            self.fallback.add(len(self.begin))
        self.begin.append(self.size); self.type.append(gt_type); self.n.append(n); self.nal.append(nal); self.amap.append(list(amap))
        self.parts.append(raw); self.size += len(raw)
        return self

    def arrays(self):
        return (b"".join(self.parts), np.array(self.begin, np.int64), np.array(self.type, np.int32), np.array(self.n, np.int32),
                np.array(self.nal, np.int32), np.array(self.amap, np.int8).reshape(-1, 5))

    def slice_bytes(self, i):
        w = bm.WIDTH.get(self.type[i], 0)
        return self.N * self.n[i] * w if self.n[i] >= 1 else 0

    def expected(self):
        """model results: rows [n_records][N] (zeros where the record is handed back), sums, statuses"""
        if getattr(self, "_expected", None) is not None:
            return self._expected
        buf, begin, gt_type, n, nal, amap = self.arrays()
        R = len(begin)
        rows, sums, status = np.zeros((R, self.N), np.uint8), np.zeros(R, np.int32), np.zeros(R, np.int32)
        for i in range(R):
            row, total, st = bm.plain_record(buf, int(begin[i]), int(gt_type[i]), int(n[i]), int(nal[i]), [int(x) for x in amap[i]], self.N)
            status[i] = st
            if st == bm.BCFIN_OK:
                rows[i], sums[i] = row, total
        self._expected = (rows, sums, status)
        return self._expected


def plain_sample(rng, n, nal):
    """n values of a sample inside the plain rule: alleles -1 .. nal - 1 either phase, a haploid call (v1 = E), nothing at all
    (v0 = E); from the third value on anything -- no value there matters"""
    v = [gt_value(int(rng.integers(-1, nal)), int(rng.integers(0, 2))) for _ in range(min(n, 2))]
    r = rng.integers(0, 12)
    if r == 0:
        v[0] = "E"                                   # then v1 is not used either: whatever it is
        if n >= 2 and rng.integers(0, 2):
            v[1] = ["M", -3, gt_value(nal)][int(rng.integers(0, 3))]
    elif r == 1 and n >= 2:
        v[1] = "E"
    v += [["E", "M", -5, gt_value(7), gt_value(0)][int(rng.integers(0, 5))] for _ in range(n - 2)]
    return v


def random_record(case, rng, gt_type=1, n=2, nal=None):
    nal = int(rng.integers(1, 6)) if nal is None else nal
    amap = MAP_ACGT if rng.integers(0, 2) else MAP_BINARY
    return case.add([plain_sample(rng, n, nal) for _ in range(case.N)], gt_type=gt_type, nal=nal, amap=amap)


SAMPLE_COUNTS = [1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000, 1031]
RECORD_COUNTS = [1, 3, 4, 5, 257, 4097]
TYPES_AND_N = [(t, n) for t in (1, 2, 3) for n in (1, 2, 3, 4)]


@functools.lru_cache(maxsize=None)
def case_samples(n_samples):
    """five records (more than one workgroup of four): int8 diploid twice, int16 diploid, int8 haploid, int32 triploid; odd gaps"""
    rng = np.random.default_rng(1000 + n_samples)
    c = Case(n_samples)
    for gt_type, n, gap in ((1, 2, 3), (1, 2, 0), (2, 2, 1), (1, 1, 7), (3, 3, 2)):
        c.pad(gap)
        random_record(c, rng, gt_type, n)
    return c


@functools.lru_cache(maxsize=None)
def case_records(n_records):
    """n_records records of 66 samples (one workgroup takes four): mostly int8 diploid, every fifth another type or ploidy"""
    rng = np.random.default_rng(2000 + n_records)
    c = Case(66)
    for i in range(n_records):
        gt_type, n = TYPES_AND_N[(i // 5) % len(TYPES_AND_N)] if i % 5 == 4 else (1, 2)
        c.pad(int(rng.integers(0, 4)))
        random_record(c, rng, gt_type, n)
    return c


@functools.lru_cache(maxsize=None)
def case_types(gt_type, n):
    rng = np.random.default_rng(3000 + 10 * gt_type + n)
    c = Case(70)
    for _ in range(3):
        c.pad(int(rng.integers(0, 5)))
        random_record(c, rng, gt_type, n)
    return c


@functools.lru_cache(maxsize=None)
def case_align():
    """slices that start at every offset 0 .. 15 behind a 16-byte boundary: int8 diploid (the 16-byte steps) and int16 / int32
    diploid, 1031 samples (rows of 1031 bytes: every row alignment too)"""
    rng = np.random.default_rng(31)
    c = Case(1031)
    for gt_type in (1, 2, 3):
        for k in range(16):
            c.pad_to(k)
            random_record(c, rng, gt_type, 2, nal=5)
    buf, begin, *_ = c.arrays()
    assert [int(b % 16) for b in begin] == list(range(16)) * 3
    return c


def _plain_rows(rng, N, n, nal):
    """samples with both alleles present (an edit of one value then decides the record)"""
    return [[gt_value(int(rng.integers(0, nal)), 1) for _ in range(n)] for _ in range(N)]


# name -> (gt_type, n, sample, value index, the value): the record is plain but for that one value.  N = 66: samples 0 .. 63 are
# taken eight at a time on the int8 diploid path, 64 and 65 one by one
VALUE_KINDS = {
    "missing_first": (1, 2, 3, 0, "M"),
    "missing_second": (1, 2, 10, 1, "M"),
    "missing_in_the_tail": (1, 2, 65, 0, "M"),
    "missing_haploid": (1, 1, 5, 0, "M"),
    "missing_int16": (2, 2, 7, 1, "M"),
    "missing_int32": (3, 2, 0, 0, "M"),
    "negative_first": (1, 2, 63, 0, -3),
    "negative_second": (1, 2, 64, 1, -1),
    "reserved_int8": (1, 2, 20, 0, -126),             # 0x82: one of the reserved values behind end-of-vector
    "negative_int16": (2, 2, 65, 0, -2),
    "int8_sentinels_in_int16": (2, 2, 9, 1, -127),    # 0xFF81 is no sentinel of int16
    "negative_int32": (3, 2, 33, 1, -2 ** 31 + 2),
    "index_is_n_alleles_first": (1, 2, 0, 0, (2 + 1) << 1),
    "index_is_n_alleles_second": (1, 2, 65, 1, (2 + 1) << 1 | 1),
    "index_127": (1, 2, 40, 0, 127),
    "wraps_to_0_as_int8_int16": (2, 2, 12, 0, (256 + 1) << 1),          # allele index 256: (int8_t)256 == 0 on the host
    "wraps_to_1_as_int8_int32": (3, 2, 64, 1, (65537 + 1) << 1),
    "wraps_to_minus_1_int16": (2, 3, 30, 0, (255 + 1) << 1),            # allele index 255: (int8_t)255 == -1 on the host
    "int8_end_byte_in_int32": (3, 2, 8, 0, 0x81),                       # 129 is an ordinary value of int32: allele index 63
}
# name -> (gt_type, n, bytes per sample): no value decides, the record as such is the caller's
RECORD_KINDS = {
    "type_float": (5, 2, 8),
    "type_char": (7, 3, 3),
    "type_none": (0, 2, 0),
    "type_int64": (4, 1, 8),
    "n_is_zero": (1, 0, 0),
}
FALLBACK_KINDS = list(VALUE_KINDS) + list(RECORD_KINDS)


@functools.lru_cache(maxsize=None)
def case_fallback(n_samples=66):
    """one record of each fallback kind between plain records (two alleles, so that index 2 is out of range)"""
    rng = np.random.default_rng(51)
    c = Case(n_samples)
    for name in FALLBACK_KINDS:
        c.pad(int(rng.integers(0, 4)))
        random_record(c, rng, 1, 2, nal=2)
        c.pad(int(rng.integers(0, 4)))
        if name in VALUE_KINDS:
            gt_type, n, s, j, v = VALUE_KINDS[name]
            vals = _plain_rows(rng, n_samples, n, 2)
            vals[s][j] = v
            c.add(vals, gt_type=gt_type, nal=2, fallback=True)
        else:
            gt_type, n, per_sample = RECORD_KINDS[name]
            c.add(raw=bytes([2]) * (per_sample * n_samples), n=n, gt_type=gt_type, nal=2, fallback=True)
    c.pad(1)
    random_record(c, rng, 1, 2, nal=2)
    return c


# edges INSIDE the plain rule: name -> (gt_type, n, sample, [(value index, value)], n_alleles)
PLAIN_EDGES = {
    "largest_index": (1, 2, 1, [(0, gt_value(4)), (1, gt_value(4, 1))], 5),
    "nothing_then_missing": (1, 2, 2, [(0, "E"), (1, "M")], 2),                   # v0 = E: v1 is not used
    "nothing_then_negative": (2, 2, 64, [(0, "E"), (1, -7)], 2),
    "nothing_then_a_large_index": (1, 2, 65, [(0, "E"), (1, gt_value(9))], 2),
    "haploid_by_end": (1, 2, 3, [(1, "E")], 2),
    "third_value_missing": (1, 3, 4, [(2, "M")], 2),
    "third_value_negative": (3, 4, 5, [(2, -9), (3, gt_value(100))], 2),
    "all_missing_alleles": (1, 2, 6, [(0, gt_value(-1)), (1, gt_value(-1, 1))], 1),
    "int16_largest": (2, 2, 7, [(0, gt_value(4)), (1, "E")], 5),
}


@functools.lru_cache(maxsize=None)
def case_plain_edges(n_samples=66):
    rng = np.random.default_rng(61)
    c = Case(n_samples)
    for name, (gt_type, n, s, edits, nal) in PLAIN_EDGES.items():
        vals = _plain_rows(rng, n_samples, n, nal)
        for j, v in edits:
            vals[s][j] = v
        c.pad(int(rng.integers(0, 4)))
        c.add(vals, gt_type=gt_type, nal=nal, amap=MAP_ACGT)
    return c


def all_cases():
    out = {"samples%d" % n: case_samples(n) for n in SAMPLE_COUNTS}
    out.update({"records%d" % n: case_records(n) for n in RECORD_COUNTS})
    out.update({"type%d_n%d" % tn: case_types(*tn) for tn in TYPES_AND_N})
    out.update(align=case_align(), fallback=case_fallback(), plain_edges=case_plain_edges())
    return out


# ---- BCF files ------------------------------------------------------------------------------------------------------------------
def typed_str(s):
    assert len(s) < 15
    return bytes([(len(s) << 4) | 7]) + s


def bcf_header(samples, contig=b"chr22", length=1000, extra=()):
    lines = [b"##fileformat=VCFv4.2", b"##FILTER=<ID=PASS,Description=\"All filters passed\",IDX=0>",
             b"##contig=<ID=%s,length=%d,IDX=0>" % (contig, length),
             b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\",IDX=1>",
             b"##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Depth\",IDX=2>",
             b"##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"PL\",IDX=3>"] + list(extra)
    lines.append(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(samples))
    text = b"\n".join(lines) + b"\n\0"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


def bcf_record(pos, alleles, n_samples, fields):
    """fields: [(dictionary index, BCF type, n, bytes of the n_samples vectors)]"""
    shared = struct.pack("<iiiIII", 0, pos - 1, 1, 0x7F800001, (len(alleles) << 16) | 0, (len(fields) << 24) | n_samples)
    shared += typed_str(b".") + b"".join(typed_str(a) for a in alleles) + bytes([0x11, 0x00])         # ID, alleles, FILTER = PASS
    indiv = b""
    for key, t, n, data in fields:
        assert n < 15
        indiv += bytes([0x11, key, (n << 4) | t]) + data
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


GT, DP, PL = 1, 2, 3
ODD_ALLELES = [b"G", b"T", b"A", b"C", b"<*>"]


def _ints(vals, w):
    return b"".join(bm.encode(x, w) for v in vals for x in v)


def _g(a, b=None, phased=1):
    return [gt_value(a), "E"] if b is None else [gt_value(a), gt_value(b, phased)]


# (position, GT type, the five samples' values, fields before GT, fields behind GT, constructed to fall back?)  --source 1
ODD_RECORDS = [
    (2, 1, [_g(0, 1), _g(1, 1, 0), _g(-1, -1, 0), _g(-1, 1), _g(4, 3)], [], [], False),
    (3, 1, [_g(0, 0), _g(1, 0), _g(2, 3), _g(3, 3, 0), _g(0, 4)], [(DP, 1, 1, _ints([[35], [3], [0], [9], [1]], 1))],
     [(PL, 2, 3, _ints([[0, 30, 300]] * 5, 2))], False),                                             # GT between two other fields
    (5, 2, [_g(0, 1), _g(1, 1), _g(-1, -1), _g(2, 3), _g(0, 4)], [], [], False),                    # int16
    (6, 3, [_g(0, 1), _g(1, 1), _g(-1, -1), _g(2, 3), _g(0, 4)], [(DP, 2, 1, _ints([[1000]] * 5, 2))], [], False),   # int32
    (7, 1, [[gt_value(0)], [gt_value(1)], [gt_value(-1)], [gt_value(4)], ["E"]], [], [], False),    # haploid: n = 1
    (8, 1, [_g(0, 1) + [gt_value(1)], _g(1, 1) + ["E"], _g(2, 2) + ["M"], _g(0) + ["E"], _g(3, 4) + [gt_value(9)]], [], [], False),   # n = 3
    (9, 1, [_g(0, 1), _g(1), _g(2), _g(3, 3), _g(4)], [], [], False),                               # mixed ploidy
    (10, 1, [_g(0, 1), ["M", gt_value(1, 1)], _g(0, 0), _g(0, 0), _g(0, 0)], [], [], True),          # the missing sentinel
    (11, 1, [_g(0, 0), _g(0, 0), _g(0, 0), [gt_value(1), -3], _g(1, 1)], [], [], True),              # a negative value
    (12, 2, [_g(0, 0), _g(1, 1), [(256 + 1) << 1, gt_value(2, 1)], _g(0, 0), _g(0, 0)], [], [], True),   # allele index 256: 0 on the host
    (13, 1, [["E", "M"], ["E", -9], _g(1, 0), _g(0, 1), _g(2, 2)], [], [(DP, 1, 1, _ints([[7]] * 5, 1))], False),   # v0 = E: v1 is not used
    (15, 1, [_g(1, 0), _g(0, 1), _g(0, 0), _g(2, 2), _g(3, 3)], [], [], False),
]


def odd_bcf():
    """(file bytes, positions constructed to fall back): five samples, five alleles G,T,A,C,<*> on every record"""
    out = [bcf_header([b"ind%d" % i for i in range(5)])]
    for pos, t, vals, before, behind, _ in ODD_RECORDS:
        n = len(vals[0])
        out.append(bcf_record(pos, ODD_ALLELES, 5, before + [(GT, t, n, _ints(vals, bm.WIDTH[t]))] + behind))
    return b"".join(out), {pos for pos, *_, fb in ODD_RECORDS if fb}


def binary_bcf(gt):
    """the BCF of packed binary genotypes gt [sites][samples] ((a1 << 4) | a0), phased int8 pairs: alleles A, C (--source 1 reads the
    nibbles back)"""
    S, N = gt.shape
    out = [bcf_header([b"ind%d" % i for i in range(N)], contig=b"chr1", length=S + 1)]
    vals = np.empty((S, N, 2), np.uint8)
    vals[:, :, 0] = ((gt & 0xF) + 1) << 1
    vals[:, :, 1] = (((gt >> 4) + 1) << 1) | 1
    for i in range(S):
        out.append(bcf_record(i + 1, [b"A", b"C"], N, [(GT, 1, 2, vals[i].tobytes())]))
    return b"".join(out)
