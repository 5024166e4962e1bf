"""Synthetic inputs of the input-parser tests: the odd-lines VCF file of the CLI tests and the line sets of the kernel tests.
Each comes with the lines that were CONSTRUCTED to fall outside the plain grammar; tests/test_vcfin_cpu.py checks that the model
sends exactly those to the host, so that a device path which falls back everywhere cannot pass the kernel tests."""
import functools

import numpy as np

import vcfin_model as vm

MAP_BINARY = [0, 1, -1, -1, -1]          # make_site's ra[] with --source 0
MAP_ACGT = [2, 3, 0, 1, 4]               # with --source 1: REF G, ALT T,A,C,<*>
ACGT_ALLELES = ["G", "T", "A", "C", "<*>"]


# ---- the odd-lines file ---------------------------------------------------------------------------------------------------------
# (position, FORMAT, the five sample columns, constructed to fall back?)  --source 1, five alleles G,T,A,C,<*> on every line
ODD_LINES = [
    (2, "GT", [".", "./.", ".|1", "0", "1/0"], False),
    (3, "GT", ["3|4", "4/3", "0|0", "2", "."], False),
    (5, "GT:DP:AD", ["0|1:35:1,2", "1|1:3:0,3", "./.:0:0,0", "2|3:9:4,5", "0/4:1:1,0"], False),
    (6, "DP:GT", ["35:0|1", "1:1|1", "0:.", "7:2/3", "12:4"], False),
    (7, "DP:AD:GT", ["35:1,2:0|1", "35", "35:1,2", "3:0,3:1|1", "."], False),            # columns with fewer subfields than gti
    (8, "GT:DP", ["0|1", "1|0:5", "0/0", "1", ".:3"], False),                              # trailing subfields dropped
    (9, "GT", ["0|1|1", "0|0", "0|0", "0|0", "0|0"], True),                                # three alleles
    (10, "GT", ["0|", "0|0", "1|1", "0|0", "0|0"], True),                                  # an empty allele
    (11, "GT", ["0|0", "001", "0|0", "0|0", "0|0"], True),                                 # more than two digits
    (12, "GT", ["01|02", "00", "4/04", "0|0", "1|1"], False),                              # two-digit indices
    (13, "GT", ["0|0", "0|0", "0|0", "0|0", "0|1\r"], True),                               # a carriage return
    (14, "GT", ["0|0", "", "0|0", "0|0", "0|0"], True),                                    # an empty column
    (15, "GT", ["1|0", "0|1", "0|0", "2|2", "3|3"], False),                                # (the last line has no newline)
]


def odd_lines_vcf():
    """(file bytes, positions constructed to fall back)"""
    out = ["##fileformat=VCFv4.2", "##contig=<ID=chr22,length=20>", "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(5))]
    for pos, fmt, cols, _ in ODD_LINES:
        out.append("chr22\t%d\t.\tG\tT,A,C,<*>\t.\tPASS\t.\t%s\t%s" % (pos, fmt, "\t".join(cols)))
    return "\n".join(out).encode(), {pos for pos, _, _, fb in ODD_LINES if fb}


# ---- line sets for the kernel ---------------------------------------------------------------------------------------------------
class Case:
    """lines of one call: text, per line (line_begin, line_end, gti, n_alleles, allele_map), n_samples, constructed fallback lines"""

    def __init__(self, n_samples):
        self.N, self.parts, self.size = n_samples, [], 0
        self.lb, self.le, self.gti, self.nal, self.amap, self.fallback = [], [], [], [], [], set()

    def add(self, cols, gti=0, nal=2, amap=MAP_BINARY, fmt=b"GT", ident=b".", fallback=False, newline=True):
        head = b"c1\t%d\t%s\tG\tT\t.\t.\t.\t%s\t" % (len(self.lb) + 1, ident, fmt)
        body = b"\t".join(cols)
        if fallback:
            self.fallback.add(len(self.lb))
        self.lb.append(self.size + len(head))
        self.le.append(self.size + len(head) + len(body))
        self.gti.append(gti); self.nal.append(nal); self.amap.append(list(amap))
        line = head + body + (b"\n" if newline else b"")
        self.parts.append(line); self.size += len(line)
        return self

    def arrays(self):
        return (b"".join(self.parts), np.array(self.lb, np.int64), np.array(self.le, np.int64), np.array(self.gti, np.int32),
                np.array(self.nal, np.int32), np.array(self.amap, np.int8).reshape(-1, 5))

    def expected(self):
        """model results: rows [n_lines][N] (zeros where the line falls back), sums, statuses"""
        if getattr(self, "_expected", None) is not None:
            return self._expected
        text, lb, le, gti, nal, amap = self.arrays()
        n = len(lb)
        rows, sums, status = np.zeros((n, self.N), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i in range(n):
            row, total, st = vm.plain_line(text, int(lb[i]), int(le[i]), int(gti[i]), int(nal[i]), [int(x) for x in amap[i]], self.N)
            status[i] = st
            if st == vm.VCFIN_OK:
                rows[i], sums[i] = row, total
        self._expected = (rows, sums, status)
        return self._expected


def _allele(rng, nal):
    r = rng.integers(0, 10)
    if r == 0:
        return b"."
    a = int(rng.integers(0, nal))
    return (b"%02d" if r == 1 else b"%d") % a


def plain_token(rng, nal):
    """a token of the plain grammar: A, A|A or A/A with one- and two-digit indices below nal"""
    r = rng.integers(0, 8)
    if r == 0:
        return _allele(rng, nal)
    return _allele(rng, nal) + (b"|" if r < 6 else b"/") + _allele(rng, nal)


def random_line(case, rng, ident=b"."):
    nal = int(rng.integers(1, 6))
    amap = MAP_ACGT if rng.integers(0, 2) else MAP_BINARY
    return case.add([plain_token(rng, nal) for _ in range(case.N)], nal=nal, amap=amap, ident=ident)


SAMPLE_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
LINE_COUNTS = [1, 3, 64, 4097]


@functools.lru_cache(maxsize=None)
def case_samples(n):
    rng = np.random.default_rng(1000 + n)
    c = Case(n)
    for _ in range(3):
        random_line(c, rng)
    return c


@functools.lru_cache(maxsize=None)
def case_lines(n_lines):
    rng = np.random.default_rng(2000 + n_lines)
    c = Case(64)
    for _ in range(n_lines):
        random_line(c, rng)
    return c


def _region_of(length, n):
    """n plain columns whose region (tokens and the tabs between them) is `length` bytes long"""
    cols = [b"0|1"] * n
    extra = length - (4 * n - 1)
    assert 0 <= extra <= 2 * n
    for k in range(extra):                         # "0|1" -> "01|1" -> "01|01"
        cols[k % n] = b"01|1" if k < n else b"01|01"
    assert sum(map(len, cols)) + n - 1 == length
    return cols


@functools.lru_cache(maxsize=None)
def case_region(length):
    """a region of exactly `length` bytes, at two alignments"""
    n = {15: 4, 16: 4, 17: 4, 4095: 1024, 4096: 1024, 4097: 1024}[length]
    c = Case(n)
    c.add(_region_of(length, n))
    c.add(_region_of(length, n), ident=b"rs12345")
    assert all(e - b == length for b, e in zip(c.lb, c.le))
    return c


REGION_LENGTHS = [15, 16, 17, 4095, 4096, 4097]


@functools.lru_cache(maxsize=None)
def case_straddle():
    """17 consecutive lines of the same 1100 columns whose ID is padded so that the region moves one byte against the 16-byte
    boundaries from line to line: it starts at each of the 16 alignments, and every lane boundary (16 bytes) and the chunk
    boundary (4096 bytes) is crossed by a token at every offset inside it"""
    rng = np.random.default_rng(31)
    c = Case(1100)
    cols = [plain_token(rng, 5) for _ in range(c.N)]
    for k in range(17):
        # the ID is padded until the region starts k bytes behind a 16-byte boundary (the text itself starts on one)
        ident = next(b"i" * n for n in range(1, 17) if (c.size + len(b"c1\t%d\t%s\tG\tT\t.\t.\t.\tGT\t" % (k + 1, b"i" * n))) % 16 == k % 16)
        c.add(cols, nal=5, amap=MAP_ACGT, ident=ident)
    text, lb, le, *_ = c.arrays()
    assert [int(b % 16) for b in lb] == [k % 16 for k in range(17)] and all(e - b > 4096 + 16 for b, e in zip(lb, le))
    return c


@functools.lru_cache(maxsize=None)
def case_gti():
    """GT as subfield 0, 1 and 2, with the trailing subfields present and dropped, and columns that end before GT"""
    rng = np.random.default_rng(41)
    c = Case(70)
    for gti in (0, 1, 2):
        for drop in (False, True):
            cols = []
            for s in range(c.N):
                tok = plain_token(rng, 4)
                sub = [b"35", b"1,2"][:gti] + [tok] + ([] if drop and s % 2 else [b"9", b"0.5,1"])
                if gti and s % 7 == 3:
                    sub = sub[:gti]                # the column ends before GT: no token
                cols.append(b":".join(sub))
            fmt = b":".join([b"DP", b"AD"][:gti] + [b"GT", b"GQ", b"XX"])
            c.add(cols, gti=gti, nal=4, amap=MAP_ACGT, fmt=fmt)
    return c


FALLBACK_KINDS = {
    "empty_allele_right": lambda cols: cols.__setitem__(2, b"0|"),
    "empty_allele_left": lambda cols: cols.__setitem__(2, b"|1"),
    "empty_column": lambda cols: cols.__setitem__(3, b""),
    "empty_last_column": lambda cols: cols.__setitem__(len(cols) - 1, b""),
    "bad_byte": lambda cols: cols.__setitem__(1, b"0|x"),
    "bad_separator": lambda cols: cols.__setitem__(1, b"0\\1"),
    "carriage_return": lambda cols: cols.__setitem__(len(cols) - 1, b"0|1\r"),
    "three_alleles": lambda cols: cols.__setitem__(0, b"0|1|1"),
    "three_digits": lambda cols: cols.__setitem__(4, b"001"),
    "dot_digit": lambda cols: cols.__setitem__(4, b".1"),
    "index_out_of_range": lambda cols: cols.__setitem__(5, b"0|2"),
    "two_digit_out_of_range": lambda cols: cols.__setitem__(5, b"10|0"),
    "one_column_less": lambda cols: cols.pop(),
    "three_columns_more": lambda cols: cols.extend([b"1|1", b"1|1", b"1|1"]),
}


@functools.lru_cache(maxsize=None)
def case_fallback(n=66):
    """one line of each fallback kind between plain lines (two alleles, so that index 2 is out of range)"""
    rng = np.random.default_rng(51)
    c = Case(n)
    kinds = []
    for name, edit in FALLBACK_KINDS.items():
        c.add([plain_token(rng, 2) for _ in range(n)])
        cols = [plain_token(rng, 2) for _ in range(n)]
        edit(cols)
        c.add(cols, fallback=True)
        kinds.append(name)
    c.add([plain_token(rng, 2) for _ in range(n)], newline=False)
    return c


def all_cases():
    out = {"samples%d" % n: case_samples(n) for n in SAMPLE_COUNTS}
    out.update({"lines%d" % n: case_lines(n) for n in LINE_COUNTS})
    out.update({"region%d" % n: case_region(n) for n in REGION_LENGTHS})
    out.update(straddle=case_straddle(), gti=case_gti(), fallback=case_fallback())
    return out
