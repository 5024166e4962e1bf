"""What the tests of fetchgl_hip --resident-bcf share (test_gpu_resident_bcf.py): the [input] line of a resident BCF file, rb_check
under the guard of miscread_util, a walk of BCF bytes in plain Python (record offsets, FORMAT fields and their data offsets) and the
damaged files of the tests."""
import os
import re
import struct
import subprocess

import miscread_util as U

RB_CHECK = os.path.join(U.ROOT, "vcfgl_amd", "bin", "rb_check")
RB_LINE = re.compile(r"\[input\] (.*?): resident-bcf (\d)(?: \((.*?)\))?, members (\d+), records (\d+), head bytes received (\d+), "
                     r"compressed bytes sent up (\d+); upload [0-9.]+ s, inflate [0-9.]+ s, chain [0-9.]+ s, heads [0-9.]+ s\n")
RB_CHECK_LINE = re.compile(r"rb_check: hops_most (\d+), head_most (\d+), total (\d+), launches (\d+), records (\d+), fields (\d+), flagged (\d)(?: \((.*?)\))?,"
                           r"(?: head bytes (\d+), GL bytes (\d+),)? differences (\d+)\n")
WIDTH = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}


def rb_line(stderr):
    m = RB_LINE.search(stderr)
    assert m, stderr[-2000:]
    return dict(resident=int(m.group(2)), why=m.group(3), members=int(m.group(4)), records=int(m.group(5)), head_bytes=int(m.group(6)), up=int(m.group(7)))


def rb_check(path, hops_most=None, head_most=None):
    args = [str(path)] + ([str(hops_most if hops_most is not None else 1 << 20)] if hops_most is not None or head_most is not None else [])
    if head_most is not None:
        args.append(str(head_most))

    def call():
        r = subprocess.run([RB_CHECK] + args, capture_output=True, text=True, timeout=U.TIMEOUT)
        return r.returncode, r.stdout, r.stderr
    rc, so, se = U.guarded("rb_check", call)
    m = RB_CHECK_LINE.search(so)
    assert m, (rc, so, se[-1500:])
    return rc, dict(hops_most=int(m.group(1)), head_most=int(m.group(2)), total=int(m.group(3)), launches=int(m.group(4)), records=int(m.group(5)),
                    fields=int(m.group(6)), flagged=int(m.group(7)), why=m.group(8), differences=int(m.group(11))), se


def _typed(b, p):
    """(type, n, p behind the descriptor)"""
    t, n = b[p] & 15, b[p] >> 4
    p += 1
    if n == 15:
        w = WIDTH[b[p] & 15]
        assert b[p] >> 4 == 1
        n = int.from_bytes(b[p + 1:p + 1 + w], "little")
        p += 1 + w
    return t, n, p


def walk(b, n_samples):
    """the records of BCF bytes: dicts of off (where the record begins), l_shared, end, fields [(key, type, n, data_off)]"""
    assert b[:5] == b"BCF\x02\x02" or b[:4] == b"BCF\x02"
    o = 9 + struct.unpack_from("<I", b, 5)[0]
    out = []
    while o < len(b):
        ls, li = struct.unpack_from("<II", b, o)
        nfs = struct.unpack_from("<I", b, o + 8 + 20)[0]
        assert nfs & 0xFFFFFF == n_samples
        p, fields = o + 8 + ls, []
        for _ in range(nfs >> 24):
            kt, kn, p = _typed(b, p)
            key = int.from_bytes(b[p:p + WIDTH[kt]], "little")
            p += WIDTH[kt] * kn
            t, n, p = _typed(b, p)
            fields.append((key, t, n, p))
            p += WIDTH[t] * n * n_samples
        assert p == o + 8 + ls + li
        out.append(dict(off=o, l_shared=ls, end=p, fields=fields))
        o = p
    return out


def header_of(b):
    """(sample names, {ID: dictionary index of every FILTER / INFO / FORMAT line}) of BCF bytes, by the rules of bcf_header: PASS is 0
    unless a FILTER line says otherwise, an IDX attribute wins, an ID seen before keeps its index"""
    text = b[9:9 + struct.unpack_from("<I", b, 5)[0]].rstrip(b"\0\n").decode()
    lines = text.split("\n")
    attr = lambda h, k: (re.search(r"[<,]%s=([^,>]*)" % k, h) or [None, ""])[1]
    keys, nd, names = {}, 0, []
    if not any(h.startswith("##FILTER=<") and attr(h, "ID") == "PASS" for h in lines):
        keys["PASS"], nd = 0, 1
    for h in lines:
        if h.startswith("#CHROM"):
            names = h.split("\t")[9:]
        if not h.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<")):
            continue
        ident, idx = attr(h, "ID"), attr(h, "IDX")
        if ident not in keys:
            keys[ident] = int(idx) if idx else nd
        nd = max(nd, keys[ident] + 1)
    return names, keys


def gl_fields(b, n_samples, gl_key=4):
    """(data_off, n) of every record's GL field (fgl_file_model.bcf_bytes: key 4)"""
    return [(f[3], f[2]) for r in walk(b, n_samples) for f in r["fields"] if f[0] == gl_key]


def patched(b, at, fmt, value):
    b = bytearray(b)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)
