"""Plain-Python statement of what the device parser of VCF sample columns computes (include/vcfgl_hip.h, "the sample columns of
VCF text"), and of what the host program's own parser (parse_record of host/vcf_input.h + make_site of host/sites.h) computes for ANY line.

    plain_line   the device's contract: (row, allelesum, VCFIN_OK) for a line inside the plain grammar, (None, None, VCFIN_HOST) else
    host_line    the host parser: the row and sum of any line it accepts (atoi on the allele bytes, int8 wrap, a1 = a0 without a
                 separator), ModelDie where the program exits
    fixed        the first nine columns of a line: pos, alleles, gti, allele_map (make_site's ra[]), offset of the sample region
    read_lines   the record lines of a file as (text, [(line_start, line_end)])

Written from the issue's semantics and from the C++ reader; it shares no code with vcfgl_amd.vcfio.
"""
import gzip

import numpy as np

VCFIN_OK, VCFIN_HOST = 0, 1
TAB, COLON, DOT, BAR, SLASH = 9, 58, 46, 124, 47


class ModelDie(Exception):
    """the host program exits with a message here"""


def read_lines(path):
    raw = (gzip.open if str(path).endswith(".gz") else open)(path, "rb").read()
    header, samples, lines, p = [], [], [], 0
    while p < len(raw):
        nl = raw.find(b"\n", p)
        le = nl if nl >= 0 else len(raw)
        if le > p:
            if raw[p:p + 2] == b"##":
                header.append(raw[p:le])
            elif raw[p:p + 1] == b"#":
                samples = raw[p:le].split(b"\t")[9:]
            else:
                lines.append((p, le))
        p = le + 1
    return raw, samples, lines


def allele_to_int(a):
    if len(a) > 1:
        return 4 if a in (b"<*>", b"<NON_REF>") else -1
    return {b"A": 0, b"C": 1, b"G": 2, b"T": 3}.get(a, -1)


def fixed(text, ls, le, source):
    """The first nine columns of the line text[ls:le].  Returns a dict; 'describable' is False where the host program hands the
    line to its own parser without asking the device (fewer than ten columns, no GT, more than five alleles, an allele that
    make_site refuses)."""
    cols, p = [], ls
    for _ in range(9):
        t = text.find(b"\t", p, le)
        if t < 0:
            return dict(describable=False, why="columns")
        cols.append(text[p:t])
        p = t + 1
    alleles = [cols[3]] + ([] if cols[4] == b"." else cols[4].split(b","))
    fmt = cols[8].split(b":")
    gti = max([i for i, k in enumerate(fmt) if k == b"GT"], default=-1)
    out = dict(pos=int(cols[1]), alleles=alleles, gti=gti, line_begin=p, n_alleles=len(alleles), describable=True)
    if gti < 0 or len(alleles) > 5 or cols[3] == b"":
        out["describable"] = False
        return out
    ra = [-1] * 5
    for i, a in enumerate(alleles):
        if source == 1:
            ra[i] = allele_to_int(a)
            ok = ra[i] != -1
        else:
            x = (a[0] if a else 0) - 48
            ok = x in (0, 1)
            ra[i] = x
        if not ok:
            out["describable"] = False
    if source == 0 and len(alleles) > 2:
        out["describable"] = False
    out["allele_map"] = ra
    return out


def _columns(text, lb, le):
    """[(start, end)] of the sample columns of the region text[lb:le]"""
    out, p = [], lb
    while True:
        t = text.find(b"\t", p, le)
        if t < 0:
            out.append((p, le))
            return out
        out.append((p, t))
        p = t + 1


def _token(text, cs, ce, gti):
    """the gti-th ':'-separated subfield of the column, or None"""
    t = cs
    for _ in range(gti):
        c = text.find(b":", t, ce)
        if c < 0:
            return None
        t = c + 1
    c = text.find(b":", t, ce)
    return text[t:(ce if c < 0 else c)]


def _plain_allele(b):
    """'.' -> -1; one or two digits -> the index; anything else -> None"""
    if b == b".":
        return -1
    if 1 <= len(b) <= 2 and all(48 <= c <= 57 for c in b):
        return int(b)
    return None


def plain_token(tok, n_alleles):
    """(a0, a1) of a token inside the plain grammar, None outside"""
    sep = min([i for i in (tok.find(b"|"), tok.find(b"/")) if i >= 0], default=-1)
    if sep < 0:
        a0 = _plain_allele(tok)
        a1 = a0
    else:
        a0, a1 = _plain_allele(tok[:sep]), _plain_allele(tok[sep + 1:])
    if a0 is None or a1 is None or a0 >= n_alleles or a1 >= n_alleles:
        return None
    return a0, a1


def _pack(a0, a1, allele_map):
    b0 = 0xF if a0 < 0 else allele_map[a0] & 0xF
    b1 = 0xF if a1 < 0 else allele_map[a1] & 0xF
    return (b1 << 4) | b0


def plain_line(text, lb, le, gti, n_alleles, allele_map, n_samples):
    """The device's contract for the sample region text[lb:le]."""
    cols = _columns(text, lb, le)
    if len(cols) != n_samples or gti < 0 or not 1 <= n_alleles <= 5:
        return None, None, VCFIN_HOST
    row, total = np.empty(n_samples, np.uint8), 0
    for s, (cs, ce) in enumerate(cols):
        tok = _token(text, cs, ce, gti)
        if tok is None:
            a0 = a1 = -1
        else:
            g = plain_token(tok, n_alleles)
            if g is None:
                return None, None, VCFIN_HOST
            a0, a1 = g
        total += max(a0, 0) + max(a1, 0)
        row[s] = _pack(a0, a1, allele_map)
    return row, total, VCFIN_OK


def _atoi_int8(b):
    """(int8_t)atoi(b): blanks, an optional sign, digits"""
    i, n = 0, len(b)
    while i < n and b[i] in (32, 9, 10, 11, 12, 13):
        i += 1
    neg = False
    if i < n and b[i] in (43, 45):
        neg = b[i] == 45
        i += 1
    v = 0
    while i < n and 48 <= b[i] <= 57:
        v = v * 10 + (b[i] - 48)
        i += 1
    v = -v if neg else v
    v &= 0xFFFFFFFF                      # (int) then (int8_t)
    v &= 0xFF
    return v - 256 if v >= 128 else v


def host_token(tok):
    """parse_record's rule for one token"""
    sep = min([i for i in (tok.find(b"|"), tok.find(b"/")) if i >= 0], default=len(tok))

    def allele(b):
        return -1 if (b == b"" or b[0] == DOT) else _atoi_int8(b)
    a0 = allele(tok[:sep])
    a1 = a0 if sep == len(tok) else allele(tok[sep + 1:])
    return a0, a1


def host_line(text, lb, le, gti, n_alleles, allele_map, n_samples):
    """parse_record + make_site for the sample region text[lb:le]: (row, allelesum); ModelDie where the program exits."""
    cols = _columns(text, lb, le)
    if len(cols) != n_samples:
        raise ModelDie("sample columns")
    row, total = np.empty(n_samples, np.uint8), 0
    for s, (cs, ce) in enumerate(cols):
        tok = _token(text, cs, ce, gti)
        a0, a1 = (-1, -1) if tok is None else host_token(tok)
        for a in (a0, a1):
            if a >= n_alleles:
                raise ModelDie("GT allele index out of range")
        total += max(a0, 0) + max(a1, 0)
        row[s] = _pack(a0, a1, allele_map)
    return row, total


def file_rows(path, source):
    """Per record line of a file: (pos, status, allelesum, row) -- the row and sum by the host's rules, the status by the device's
    grammar.  What `vcfgl_hip --dump-gt FILE SOURCE x` prints."""
    text, samples, lines = read_lines(path)
    n, out = len(samples), []
    for ls, le in lines:
        f = fixed(text, ls, le, source)
        if not f["describable"]:
            raise ModelDie("fixed columns")
        _, _, st = plain_line(text, f["line_begin"], le, f["gti"], f["n_alleles"], f["allele_map"], n)
        row, total = host_line(text, f["line_begin"], le, f["gti"], f["n_alleles"], f["allele_map"], n)
        out.append((f["pos"], st, total, row))
    return out


def dump_text(rows):
    return "".join("%d %d %d %s\n" % (pos, st, total, bytes(row).hex()) for pos, st, total, row in rows)
