"""What the tests of --device-inflate and --resident share (test_miscread_cli_cpu.py, test_gpu_miscread.py, test_gpu_resident.py):
the programs under a timeout with a stop after the first one that faults, the [input] lines of --verbose 1, BGZF containers and
their damaged forms, and VCF texts built around given byte offsets."""
import gzip
import os
import re
import subprocess

import pytest

import fgl_file_model as gm
from vcfgl_amd import discordance as D
from vcfgl_amd import fetchgl as F
from vcfgl_amd import setalleles as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_CHECK = os.path.join(ROOT, "vcfgl_amd", "bin", "rf_check")
TIMEOUT = 120
DEAD = (-6, -11, 134, 139, 124, 137)
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started

INFLATE_LINE = re.compile(r"\[input\] (.*?): device-inflate 1, members inflated on the device (\d+), bytes sent up (\d+), received (\d+), "
                          r"inflate [0-9.]+ s, read by the host: (no|yes)(?: \((.*)\))?\n")
RESIDENT_LINE = re.compile(r"\[input\] (.*?): resident (\d)(?: \((.*?)\))?, RF_CHUNK (\d+), members (\d+), lines (\d+), head bytes received (\d+), "
                           r"compressed bytes sent up (\d+); upload [0-9.]+ s, inflate [0-9.]+ s, split [0-9.]+ s\n")
FETCH_LINE = re.compile(r"\[fetchgl\] on-device (\d): records (\d+), with a CSV line (\d+), redone on the host (\d+), bytes sent up (\d+), received (\d+)")


def guarded(what, call):
    """runs a GPU process through `call` -> (rc, stdout, stderr); after one that died nothing more is started"""
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        r = call()
    except subprocess.TimeoutExpired:
        _gave_up.append(what + " (timeout)")
        pytest.fail("%s ran out of time: no further GPU process is started" % what)
    if r[0] in DEAD:
        _gave_up.append(what)
        pytest.fail("%s ended with status %d: no further GPU process is started" % (what, r[0]))
    return r


def fetch(path, gt, **kw):
    kw.setdefault("verbose", True)
    return guarded("fetchgl_hip", lambda: F.fetch_file(path, gt, timeout=TIMEOUT, **kw))


def set_alleles(path, tsv, prefix, mode, **kw):
    return guarded("setalleles_hip", lambda: S.set_file(path, tsv, prefix, mode, verbose=True, timeout=TIMEOUT, **kw))


def compare(truth, call, out, **kw):
    return guarded("gtdiscordance_hip", lambda: D.compare_files(truth, call, out, verbose=True, timeout=TIMEOUT, **kw))


def rf_check(path, head_most=None):
    def call():
        r = subprocess.run([RF_CHECK, str(path)] + ([str(head_most)] if head_most is not None else []), capture_output=True, text=True, timeout=TIMEOUT)
        return r.returncode, r.stdout, r.stderr
    return guarded("rf_check", call)


def plain(stderr):
    """stderr without the tools' own [...] lines of --verbose 1"""
    return "".join(ln for ln in stderr.splitlines(True) if not ln.startswith(("[input]", "[fetchgl]", "[setalleles]", "[gtdisc]")))


def inflate_lines(stderr):
    return [dict(file=m.group(1), members=int(m.group(2)), up=int(m.group(3)), down=int(m.group(4)), host=m.group(5) == "yes", why=m.group(6))
            for m in INFLATE_LINE.finditer(stderr)]


def resident_line(stderr):
    m = RESIDENT_LINE.search(stderr)
    assert m, stderr[-2000:]
    return dict(resident=int(m.group(2)), why=m.group(3), chunk=int(m.group(4)), members=int(m.group(5)), lines=int(m.group(6)), head_bytes=int(m.group(7)),
                up=int(m.group(8)))


def fetch_counts(stderr):
    m = FETCH_LINE.search(stderr)
    assert m, stderr[-2000:]
    return tuple(int(m.group(k)) for k in (2, 3, 4, 5, 6))


def write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def damaged(text):
    """name -> (bytes of the file, what the [input] line must say): containers that are not a clean series of BGZF members"""
    z = gm.bgzf(text, block=3000)
    first = int.from_bytes(z[16:18], "little") + 1 - 8                 # where the first member's CRC32 begins (BSIZE + 1 bytes a member)
    flipped = bytearray(z)
    flipped[first] ^= 0x40
    not_bgzf, left = "not a series of BGZF members", "left to the host"
    return {"plain": (text, not_bgzf), "gzip": (gzip.compress(text), not_bgzf), "crc": (bytes(flipped), left),
            "truncated": (z[:-40], not_bgzf), "trailing": (z + b"xyz", not_bgzf)}


# ---- VCF text around byte offsets --------------------------------------------------------------------------------------------------
HEAD = ['##fileformat=VCFv4.2', '##contig=<ID=chr22,length=2147483647>', '##FORMAT=<ID=GL,Number=G,Type=Float,Description="GL">']


def names_line(n):
    return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % s for s in range(n))


def record(pos, n, ident=".", info=".", columns=9):
    """a record line without its '\\n': REF A, ALT C, FORMAT GL, `n` samples of three values"""
    head = ["chr22", str(pos), ident, "A", "C", ".", "PASS", info, "GL"][:columns]
    cols = ["-%d.%d,-0.25,-%d" % (1 + (pos + s) % 7, s % 10, 3 + s % 5) for s in range(n)] if columns == 9 else []
    return "\t".join(head + cols)


def text_with(n, n_before, place, offset, n_after=2):
    """header, `n_before` records, then a record whose ID column is as long as it takes to put its `place` -- 'newline' (the line's
    last byte), 'tab9' (the ninth tab) or 'begin' (the first byte of the record behind it) -- at byte `offset`; `n_after` records follow"""
    lines = HEAD + [names_line(n)] + [record(10 + i, n) for i in range(n_before)]
    at = len("\n".join(lines)) + 1
    probe = record(500, n, ident="")
    where = {"newline": len(probe), "tab9": probe.index("\tGL\t") + 3, "begin": len(probe) + 1}[place]
    fill = offset - at - where
    assert fill >= 1, (fill, "the offset lies before the record can reach it")
    lines.append(record(500, n, ident="i" * fill))
    text = "\n".join(lines + [record(600 + i, n) for i in range(n_after)]) + "\n"
    b = text.encode()
    assert {"newline": b[offset:offset + 1] == b"\n", "tab9": b[offset:offset + 1] == b"\t" and b[:offset].split(b"\n")[-1].count(b"\t") == 8,
            "begin": b[offset - 1:offset] == b"\n"}[place]
    return b


def text_of_length(n, total, newline=True):
    """a file of exactly `total` bytes: the last record's ID column takes what is left"""
    lines = HEAD + [names_line(n)] + [record(10 + i, n) for i in range(3)]
    at = len("\n".join(lines)) + 1
    fill = total - at - len(record(500, n, ident="")) - (1 if newline else 0)
    assert fill >= 1
    b = ("\n".join(lines + [record(500, n, ident="j" * fill)]) + ("\n" if newline else "")).encode()
    assert len(b) == total
    return b
