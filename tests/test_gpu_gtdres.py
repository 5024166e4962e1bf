"""gtdiscordance_hip --resident 1 (both files of the pair inflated into GPU memory and left there: the heads alone come down, the
batches' descriptors point into the files, k_gtd_parse / k_gtd_bcf_decode read each side from a base of its own): every byte the run
writes -- the output file, the -perSite lines on stdout, the tool's lines on stderr, the exit status -- is what the same binary writes
with --on-device 0 --device-inflate 0 (the host path, which the CPU tests hold to tests/gtdisc_model.py and the recorded outputs),
and what --resident 0 writes on the device.

A test does not pass by falling back: where the files are meant to be resident both [input] lines must say `resident 1`, and `redone
on the host` must be the number of records the model (gtdbcf_cases.not_plain) finds outside the plain rules -- 0 for the plain shapes.

Generators: tests/gtdisc_model.py (write_pair) and the BCF writer of tests/gtdbcf_cases.py; small text builders of its own put a
line's '\\n', ninth tab and first sample byte around RF_CHUNK.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import gzip
import os
import re

import pytest

import gtdbcf_cases as gc
import gtdisc_model as gm
import miscread_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_gtdiscordance")
E, M = gc.E, gc.M
INPUT = re.compile(r"\[input\] (\S+): resident (\d)(?: \((.*?)\))?, (?:RF_CHUNK (\d+), )?members (\d+), (lines|records) (\d+), head bytes received (\d+), "
                   r"compressed bytes sent up (\d+); upload [0-9.]+ s, inflate [0-9.]+ s, (?:split|chain) [0-9.]+ s")
GTDISC = re.compile(r"\[gtdisc\] on-device 1: records (\d+), redone on the host (\d+), text bytes sent up (\d+);")
BCF = re.compile(r"\[bcf\] .*?vector bytes sent up (\d+), text bytes sent up (\d+);")
STAGE = re.compile(r"\[resident\] truth (\d), call (\d): device stage ([0-9.]+) ms over (\d+) batches \(hipEvent pairs\), of which (k_gtd_parse|k_gtd_bcf_decode) ([0-9.]+) ms")


class Got:
    def __init__(self, rc, so, se, out):
        self.rc, self.stdout, self.raw = rc, so, se
        self.out = open(out, "rb").read() if os.path.exists(out) else None
        text = "".join(ln for ln in se.splitlines(True) if not ln.startswith(("[gtdisc]", "[bcf]", "[input]", "[resident]"))).replace(out, "OUT")
        self.text = re.sub(r"truth file \S+ and the call file \S+", "truth file T and the call file C", text)
        self.inputs = [dict(resident=int(m.group(2)), why=m.group(3), members=int(m.group(5)), kind=m.group(6), n=int(m.group(7)), head=int(m.group(8)), up=int(m.group(9)))
                       for m in INPUT.finditer(se)]
        m = GTDISC.search(se)
        self.records, self.redone, self.text_up = (int(m.group(k)) for k in (1, 2, 3)) if m else (None, None, None)
        m = BCF.search(se)
        self.vec_up = int(m.group(1)) if m else 0
        self.stage = STAGE.search(se)

    def same(self, want):
        assert self.rc == want.rc, (self.text[-1500:], want.text[-1500:])
        assert self.out == want.out and self.stdout == want.stdout and self.text == want.text, (self.text[-1500:], want.text[-1500:])


def _run(tmp_path, name, truth, call, **kw):
    out = str(tmp_path / (name + ".tsv"))
    if os.path.exists(out):
        os.remove(out)
    rc, so, se = U.compare(truth, call, out, **kw)
    return Got(rc, so, se, out)


def host(tmp_path, truth, call, **kw):
    """the yardstick: the same binary on the host, zlib reading the files"""
    kw.pop("batch_records", None)
    return _run(tmp_path, "host", truth, call, on_device=False, device_inflate=False, **kw)


def staged(tmp_path, truth, call, **kw):
    """the second yardstick: --resident 0 on the device"""
    return _run(tmp_path, "staged", truth, call, on_device=True, device_inflate=True, resident=False, **kw)


def resident(tmp_path, truth, call, both=True, **kw):
    got = _run(tmp_path, "resident", truth, call, on_device=True, device_inflate=True, resident=True, **kw)
    if both:
        assert [i["resident"] for i in got.inputs] == [1, 1] and [i["why"] for i in got.inputs] == [None, None], got.raw[-2000:]
        assert all(i["members"] > 0 and i["up"] > 0 and i["head"] > 0 for i in got.inputs)
        assert "device-inflate 1, members inflated" not in got.raw           # no part of a file came down whole
        assert got.rc != 0 or (got.text_up == 0 and got.vec_up == 0)        # descriptors alone go up
    return got


def write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def bgz(tmp_path, name, src, block=4000, eof=True):
    data = src if isinstance(src, bytes) else open(src, "rb").read()
    z = gc.bgzf(data, block=block)
    return write(tmp_path / name, z if eof else z[:-28])


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]
BATCHES = (1, 7, 4096)
_shape_cache = {}


def _mode(k, j):
    return (3 * k + j) % 9               # every -doGQ 0 .. 8 over the 45 cases


def _shape(tmp_path_factory, k, fmt):
    """the pair of shape k as text and as BCF, both BGZF: made once per FORMAT"""
    if (k, fmt) not in _shape_cache:
        n, r = SHAPES[k]
        d = tmp_path_factory.mktemp("gtdres_shape%d" % k)
        for seed in range(6000 + k, 7000, 100):                             # (the first seed that gives the truth file records of its own)
            p = gc.pair_from_generator(d, "s%d" % seed, n, r, fmt, seed=seed, first_pos=(8 if k % 2 else 2 ** 31 - 1000))
            if len(gm.parse(p.t_vcf)[2]) > r:
                break
        block = (300, 4096, 60000)[k % 3]
        files = dict(tt=bgz(d, "t.vcf.gz", p.t_vcf, block), ct=bgz(d, "c.vcf.gz", p.c_vcf, block, eof=k % 2 == 0),
                     tb=bgz(d, "t.bcf.gz", p.t_bcf, block, eof=k % 2 == 1), cb=bgz(d, "c.bcf.gz", p.c_bcf, block))
        assert len(gm.parse(p.t_vcf)[2]) > r                                # truth records the call file lacks: paired offsets are not contiguous
        _shape_cache[(k, fmt)] = (p, files)
    return _shape_cache[(k, fmt)]


@pytest.mark.parametrize("j", range(3))
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_shapes_batches_and_modes(k, j, tmp_path, tmp_path_factory):
    n, r = SHAPES[k]
    mode = _mode(k, j)
    fmt = "GT:PL" if mode == 8 and k % 2 else "GT:PL:GQ" if mode >= 7 else "GT:GQ"      # (-doGQ 8 reads PL only without a GQ header)
    p, f = _shape(tmp_path_factory, k, fmt)
    kw = dict(do_gq=mode, per_site=True, batch_records=BATCHES[j])
    assert p.not_plain(mode) == (0, r)                                      # all plain, says the model: nothing may be handed back
    want = host(tmp_path, f["tt"], f["ct"], **kw)
    assert want.rc == 0 and len(want.out) > 0 and len(want.stdout) > 0, want.text[-1500:]
    got = resident(tmp_path, f["tt"], f["ct"], **kw)
    got.same(want)
    assert (got.records, got.redone) == (r, 0) and [i["kind"] for i in got.inputs] == ["lines", "lines"]
    assert got.stage and got.stage.group(5) == "k_gtd_parse" and got.stage.group(4) == str(-(-r // min(BATCHES[j], r)))
    got = resident(tmp_path, f["tb"], f["cb"], bcf_direct=True, **kw)
    got.same(want)
    assert (got.records, got.redone) == (r, 0) and [i["kind"] for i in got.inputs] == ["records", "records"] and got.inputs[1]["n"] == r
    assert got.stage and got.stage.group(5) == "k_gtd_bcf_decode"


# ---- members --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtdres_odd")
    return gc.pair_from_generator(d, "m", 65, 60, "GT:PL:GQ", seed=11, odd_share=0.1)


@pytest.mark.parametrize("block,eof", [(300, True), (4096, False), (60000, True), (60000, False)])
def test_lines_and_vectors_across_members(block, eof, odd_pair, tmp_path):
    p = odd_pair
    kw = dict(do_gq=2, per_site=True, batch_records=16)
    nonplain = p.not_plain(2)[0]
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    assert want.rc == 0 and nonplain > 0
    for t, c, direct in ((bgz(tmp_path, "t.vcf.gz", p.t_vcf, block, eof), bgz(tmp_path, "c.vcf.gz", p.c_vcf, block, eof), None),
                         (bgz(tmp_path, "t.bcf.gz", p.t_bcf, block, eof), bgz(tmp_path, "c.bcf.gz", p.c_bcf, block, eof), True)):
        got = resident(tmp_path, t, c, bcf_direct=direct, **kw)
        got.same(want)
        assert (got.records, got.redone) == (60, nonplain)
        assert got.inputs[0]["members"] == -(-os.path.getsize(p.t_bcf if direct else p.t_vcf) // block) + (1 if eof else 0)


def test_more_members_than_one_inflate_call(tmp_path):
    """members of 5 and 3 bytes: more than the 512 of a batch of the staged reader and more than the 4096 of a call of the resident one"""
    p = gc.pair_from_generator(tmp_path, "mm", 65, 100, "GT:GQ", seed=12)
    kw = dict(do_gq=6, per_site=True)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    got = resident(tmp_path, bgz(tmp_path, "t.vcf.gz", p.t_vcf, 5), bgz(tmp_path, "c.bcf.gz", p.c_bcf, 3), bcf_direct=True, **kw)
    got.same(want)
    assert want.rc == 0 and (got.records, got.redone) == (100, 0) and min(i["members"] for i in got.inputs) > 4096


# ---- chunks, text ---------------------------------------------------------------------------------------------------------------------
HEAD = ["##fileformat=VCFv4.2", "##contig=<ID=chr1,length=4294967295>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
        '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">']


def names_line(n):
    return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % s for s in range(n))


def line(pos, n, call, ident=".", cols=None):
    """a plain record line without its '\\n': REF A, ALT C,G,T; truth columns a/b, call columns a|b:GQ"""
    if cols is None:
        cols = [("%d|%d:%d" % ((pos + s) % 4, (pos + 2 * s) % 4, 1 + (pos + s) % 127)) if call else ("%d/%d" % ((pos + s) % 4, (3 * pos + s) % 4)) for s in range(n)]
    return "\t".join(["chr1", str(pos), ident, "A", "C,G,T", ".", "PASS", ".", "GT:GQ" if call else "GT"] + cols)


def text_with(n, call, place, offset, positions=(10, 11, 12, 13, 14, 15), at=3):
    """the records at `positions`; the one at index `at` has an ID column as long as it takes to put its `place` -- 'newline' (the
    line's last byte), 'tab9' (the ninth tab) or 'sample' (the first byte of its sample columns) -- at byte `offset` of the text"""
    lines = HEAD + [names_line(n)] + [line(p, n, call) for p in positions[:at]]
    begin = len("\n".join(lines)) + 1
    probe = line(positions[at], n, call, ident="")
    tab9 = len("\t".join(probe.split("\t")[:9]))
    where = {"newline": len(probe), "tab9": tab9, "sample": tab9 + 1}[place]
    fill = offset - begin - where
    assert fill >= 1, (fill, "the offset lies before the record can reach it")
    lines.append(line(positions[at], n, call, ident="i" * fill))
    b = ("\n".join(lines + [line(p, n, call) for p in positions[at + 1:]]) + "\n").encode()
    assert b[offset:offset + 1] == (b"\n" if place == "newline" else b"\t" if place == "tab9" else line(positions[at], n, call).split("\t")[9][:1].encode())
    assert place != "tab9" or b[:offset].split(b"\n")[-1].count(b"\t") == 8
    return b


def plain_text(n, call, positions, newline=True, empty_at=None):
    lines = HEAD + [names_line(n)] + [line(p, n, call) for p in positions]
    if empty_at is not None:
        lines.insert(len(HEAD) + 1 + empty_at, "")
    return ("\n".join(lines) + ("\n" if newline else "")).encode()


@pytest.fixture(scope="module")
def chunk(tmp_path_factory):
    """RF_CHUNK as the program prints it"""
    d = tmp_path_factory.mktemp("gtdres_chunk")
    t, c = bgz(d, "t.vcf.gz", plain_text(2, False, (10, 11))), bgz(d, "c.vcf.gz", plain_text(2, True, (10, 11)))
    got = resident(d, t, c)
    m = re.search(r"RF_CHUNK (\d+),", got.raw)
    assert got.rc == 0 and m and int(m.group(1)) >= 64
    return int(m.group(1))


TRUTH_POS, CALL_POS = (8, 10, 11, 12, 13, 14, 15, 16), (10, 11, 13, 14, 15)        # truth records in front, between and behind


@pytest.mark.parametrize("place", ["newline", "tab9", "sample"])
@pytest.mark.parametrize("side", ["truth", "call"])
def test_a_line_around_a_chunk_boundary(side, place, chunk, tmp_path):
    n = 3
    for d in (-1, 0, 1):
        offset = 2 * chunk + d
        t = text_with(n, False, place, offset, TRUTH_POS, at=4) if side == "truth" else plain_text(n, False, TRUTH_POS)
        c = text_with(n, True, place, offset, CALL_POS, at=2) if side == "call" else plain_text(n, True, CALL_POS)
        tz, cz = bgz(tmp_path, "t%d.vcf.gz" % d, t, 1500), bgz(tmp_path, "c%d.vcf.gz" % d, c, 1500)
        kw = dict(do_gq=2, per_site=True, batch_records=2)
        want = host(tmp_path, tz, cz, **kw)
        got = resident(tmp_path, tz, cz, **kw)
        got.same(want)
        assert want.rc == 0 and (got.records, got.redone) == (5, 0) and want.stdout.count("\n") == 5 * n
        assert [i["n"] for i in got.inputs] == [t.count(b"\n"), c.count(b"\n")]


@pytest.mark.parametrize("side", ["truth", "call", "both"])
def test_a_last_line_without_newline_and_an_empty_line(side, tmp_path):
    n = 65
    t = plain_text(n, False, TRUTH_POS[:-1], newline=side == "call", empty_at=None if side == "call" else 2)      # (the last truth record is compared)
    c = plain_text(n, True, CALL_POS, newline=side == "truth", empty_at=None if side == "truth" else 1)
    tz, cz = bgz(tmp_path, "t.vcf.gz", t, 700), bgz(tmp_path, "c.vcf.gz", c, 700)
    kw = dict(do_gq=6, per_site=True, batch_records=2)
    want = host(tmp_path, tz, cz, **kw)
    got = resident(tmp_path, tz, cz, **kw)
    got.same(want)
    assert want.rc == 0 and (got.records, got.redone) == (5, 0)
    assert got.inputs[1]["n"] == c.count(b"\n") + (0 if c.endswith(b"\n") else 1)


# ---- vectors, BCF ---------------------------------------------------------------------------------------------------------------------
def _gt_fields(t, gq_t=1, wide_at=None):
    def fields(rnd, i, tg, nal):
        gt = [[gc.gt_value(a), gc.gt_value(b, rnd.randrange(2))] for a, b in tg]
        for v in gt:
            if rnd.random() < 0.1:
                v[rnd.randrange(2)] = rnd.choice((M, gc.gt_value(-1)))
        if wide_at == i:
            gt[len(gt) // 2] = [gc.gt_value(70), gc.gt_value(0)]            # an index a writer needs int16 for: not plain (above the sixteen of the map)
        return [("GT", 2 if wide_at == i else t, 2, gt), ("GQ", gq_t, 1, [[rnd.choice((1, 9, 10, 99, 100, 127))] for _ in tg])]
    return fields


def spread_ids(samples, trecs, crecs, has_gq=True, has_pl=False):
    """gives every record an ID of 0 .. 15 characters (fifteen take a length of three bytes), chosen one record after the other so that the GT vectors of both files start
    at as many addresses mod 16 as they can; returns the residues reached (truth, call)"""
    seen = (set(), set())
    flags = ((False, False), (has_gq, has_pl))
    at = [len(gc.bcf_bytes(samples, [], *f)) for f in flags]
    for i in range(len(trecs)):
        size, gt = [], []
        for recs, f in zip((trecs, crecs), flags):
            recs[i].rid = ""
            one = gc.bcf_bytes(samples, [recs[i]], *f)
            size.append(len(one) - len(gc.bcf_bytes(samples, [], *f)))
            gt.append(gc.vector_offsets(samples, [recs[i]], "GT", *f)[0] - len(gc.bcf_bytes(samples, [], *f)))
        grow = lambda L: L + (2 if L == 15 else 0)
        best = max(range(16), key=lambda L: (sum((at[k] + gt[k] + grow(L)) % 16 not in seen[k] for k in (0, 1)), L == (i % 16)))
        for k, recs in enumerate((trecs, crecs)):
            recs[i].rid = "r" * best
            seen[k].add((at[k] + gt[k] + grow(best)) % 16)
            at[k] += size[k] + grow(best)
    return seen


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 257])
def test_gt_vectors_at_every_residue_of_sixteen(n, t, tmp_path):
    """ID lengths 0 .. 15 move the GT vectors of both files through every address mod 16; the truth file's last vector ends the file,
    so the aligned piece behind it lies outside"""
    samples, trecs, crecs = gc.simple_pair(tmp_path, "v", n, 24, 300 + n, _gt_fields(t), truth_type=t)
    assert spread_ids(samples, trecs, crecs) == (set(range(16)), set(range(16)))
    p = gc.Pair(tmp_path, "v", samples, trecs, crecs, has_pl=False)
    assert {x % 16 for x in gc.vector_offsets(samples, trecs, "GT", False, False)} == set(range(16))
    assert gc.vector_offsets(samples, trecs, "GT", False, False)[-1] + 2 * t * n == os.path.getsize(p.t_bcf)
    kw = dict(do_gq=6, per_site=True, batch_records=5)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    got = resident(tmp_path, p.t_bgzf, p.c_bgzf, bcf_direct=True, **kw)
    got.same(want)
    assert want.rc == 0 and p.not_plain(6) == (0, 24) and (got.records, got.redone) == (24, 0)
    staged(tmp_path, p.t_bgzf, p.c_bgzf, bcf_direct=True, **kw).same(want)


def test_an_allele_index_of_int16_is_handed_back(tmp_path):
    al = ["A", "C", "G", "T"] + ["A%d" % k for k in range(96)]
    samples, trecs, crecs = gc.simple_pair(tmp_path, "w", 9, 17, 41, _gt_fields(1, wide_at=8), ids=lambda i: "r" * (i % 17), alleles=lambda i: al)
    p = gc.Pair(tmp_path, "w", samples, trecs, crecs, has_pl=False)
    kw = dict(do_gq=6, per_site=True, batch_records=5)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    got = resident(tmp_path, p.t_bgzf, p.c_bgzf, bcf_direct=True, **kw)
    got.same(want)
    assert p.not_plain(6) == (1, 17) and (got.records, got.redone) == (17, 1)


def _pl_fields(pl_t):
    def fields(rnd, i, tg, nal):
        nG = nal * (nal + 1) // 2
        gt, pl = [], []
        for a, b in tg:
            gt.append([gc.gt_value(-1), gc.gt_value(-1)] if rnd.random() < 0.15 else [gc.gt_value(a), gc.gt_value(b, 1)])
            v = [rnd.choice((3, 17, 60, 126, 0)) if pl_t == 1 else rnd.choice((3, 17, 126, 127, 128, 255, 1000, 9999, 0)) for _ in range(nG)]
            v[rnd.randrange(nG)] = M if rnd.random() < 0.2 else 0
            pl.append(v)
        return [("GT", 1, 2, gt), ("PL", pl_t, nG, pl)]
    return fields


@pytest.mark.parametrize("pl_t", [1, 2, 3])
@pytest.mark.parametrize("nal", [1, 2, 3, 4, 5])
def test_doGQ_8_reads_pl_where_it_lies(nal, pl_t, tmp_path):
    samples, trecs, crecs = gc.simple_pair(tmp_path, "pl", 66, 6, 50 + nal, _pl_fields(pl_t), nal=nal, ids=lambda i: "q" * (3 * i))
    p = gc.Pair(tmp_path, "pl", samples, trecs, crecs, has_gq=False)
    kw = dict(do_gq=8, per_site=True, batch_records=4)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    got = resident(tmp_path, p.t_bgzf, p.c_bgzf, bcf_direct=True, **kw)
    got.same(want)
    assert want.rc == 0 and p.not_plain(8) == (0, 6) and (got.records, got.redone) == (6, 0), got.text[-1500:]


# ---- pairs ----------------------------------------------------------------------------------------------------------------------------
def test_text_and_bcf_in_every_pairing(odd_pair, tmp_path):
    p = odd_pair
    tt, ct = bgz(tmp_path, "t.vcf.gz", p.t_vcf), bgz(tmp_path, "c.vcf.gz", p.c_vcf)
    for m in (dict(do_gq=2, per_site=True), dict(do_gq=8)):
        kw = dict(batch_records=16, **m)
        want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
        nonplain = p.not_plain(m["do_gq"])[0]
        assert want.rc == 0 and nonplain > 0
        for t, c in ((tt, ct), (p.t_bgzf, p.c_bgzf), (p.t_bgzf, ct), (tt, p.c_bgzf)):
            got = resident(tmp_path, t, c, bcf_direct=True, **kw)
            got.same(want)
            assert (got.records, got.redone) == (60, nonplain)
            assert [i["kind"] for i in got.inputs] == ["records" if t == p.t_bgzf else "lines", "records" if c == p.c_bgzf else "lines"]
        staged(tmp_path, p.t_bgzf, ct, bcf_direct=True, **kw).same(want)


def test_one_file_resident_and_one_not(odd_pair, tmp_path):
    p = odd_pair
    tt, ct = bgz(tmp_path, "t.vcf.gz", p.t_vcf), bgz(tmp_path, "c.vcf.gz", p.c_vcf)
    kw = dict(do_gq=2, per_site=True, batch_records=16, bcf_direct=True)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    nonplain = p.not_plain(2)[0]
    truth_bytes = os.path.getsize(tt) + os.path.getsize(p.t_vcf)
    cases = [(tt, p.c_vcf, None, [1, 0], "not a series of BGZF members"),            # a plain-text call file
             (p.t_bcf, p.c_bgzf, None, [0, 1], "not a series of BGZF members"),      # a raw BCF truth file
             (p.t_bgzf, p.c_vcf, None, [1, 0], "not a series of BGZF members"),
             (tt, ct, truth_bytes, [1, 0], "exceed what --resident-max-bytes leaves"),   # the bound admits the truth file only
             (tt, p.c_bgzf, truth_bytes + 100, [1, 0], "exceed what --resident-max-bytes leaves")]
    for t, c, most, res, why in cases:
        got = resident(tmp_path, t, c, both=False, resident_max_bytes=most, **kw)
        got.same(want)
        assert [i["resident"] for i in got.inputs] == res, got.raw[-2000:]
        assert why in got.inputs[res.index(0)]["why"] and got.inputs[res.index(1)]["why"] is None
        assert (got.records, got.redone) == (60, nonplain)
        assert got.text_up + got.vec_up > 0                                 # the side that is not resident is staged


# ---- handed back ----------------------------------------------------------------------------------------------------------------------
ODD = {"call_three_digits": ("call", "001|1:30", 0), "call_gq_0": ("call", "0/1:0", 1), "call_three_alleles": ("call", "0/1/2:30", 1),
       "truth_three_digits": ("truth", "002/1", 0), "truth_missing": ("truth", "./.", 1), "both_three_digits": ("both", None, 0)}


@pytest.mark.parametrize("kind", sorted(ODD))
def test_text_records_for_the_host_at_each_place_of_a_batch(kind, tmp_path):
    side, token, rc = ODD[kind]
    n, pos = 5, list(range(20, 34))
    for at in (0, 3, 6):                                                    # batches of 7: the first, a middle and the last record of the first batch
        tl = [line(q, n, False) for q in [19] + pos + [40]]
        cl = [line(q, n, True) for q in pos]
        if side in ("truth", "both"):
            f = tl[1 + at].split("\t"); f[10] = token or "002/1"; tl[1 + at] = "\t".join(f)
        if side in ("call", "both"):
            f = cl[at].split("\t"); f[10] = token or "001|1:30"; cl[at] = "\t".join(f)
        body = "\n".join(HEAD + [names_line(n)]) + "\n"
        tz = bgz(tmp_path, "t%d.vcf.gz" % at, (body + "\n".join(tl) + "\n").encode(), 500)
        cz = bgz(tmp_path, "c%d.vcf.gz" % at, (body + "\n".join(cl) + "\n").encode(), 500)
        kw = dict(do_gq=2, per_site=True, batch_records=7)
        want = host(tmp_path, tz, cz, **kw)
        got = resident(tmp_path, tz, cz, **kw)
        got.same(want)
        assert want.rc == rc, want.text[-1000:]
        if rc == 0:
            assert (got.records, got.redone) == (14, 1) and want.stdout.count("\n") == 14 * n
        else:
            assert want.stdout.count("\n") == at * n + 1                    # the records before it, and the sample before the one that stops
        staged(tmp_path, tz, cz, **kw).same(want)


BCF_ODD = ["missing_beside_three_digits", "pl_of_five_digits", "allele_sixteen", "three_alleles", "one_allele", "gq_128", "pl_too_few", "pl_too_many",
           "truth_allele_sixteen", "both_allele_sixteen"]
BCF_ODD_STOPS = {"three_alleles": 1, "one_allele": 1, "gq_128": 1, "pl_too_few": 0, "pl_too_many": 0}      # the run stops: samples of the record listed before


@pytest.mark.parametrize("kind", BCF_ODD)
def test_bcf_records_for_the_host_at_each_place_of_a_batch(kind, tmp_path):
    """every kind of sample the README row of --bcf-direct lists, in the call record, the truth record or both"""
    mode = 8 if kind.startswith("pl_") else 6
    al17 = ["A", "C", "G", "T"] + ["<N%d>" % k for k in range(12)] + ["AT"]
    for at in (0, 3, 6):
        def fields(rnd, i, tg, nal):
            gt = [[gc.gt_value(a), gc.gt_value(b, 1)] for a, b in tg]
            gq = [[rnd.randint(1, 127)] for _ in tg]
            pl = [[0, 20, 200] + [300] * (nal * (nal + 1) // 2 - 3) for _ in tg]
            t, k, gq_t = 1, 2, 1
            if i == at and kind == "missing_beside_three_digits":
                gt[1], t = [gc.gt_value(-1), gc.gt_value(117)], 2
            if i == at and kind == "pl_of_five_digits":
                gt[1], pl[1][2] = [gc.gt_value(-1), gc.gt_value(0)], 10000
            if i == at and kind in ("allele_sixteen", "both_allele_sixteen"):
                gt[1] = [gc.gt_value(16), gc.gt_value(0)]
            if i == at and kind == "one_allele":
                gt[1] = [gc.gt_value(0), E]
            if i == at and kind == "pl_too_few":
                pl[1][-1] = E
            if i == at and kind == "pl_too_many":
                pl = [v + [E] for v in pl]
                pl[1][-1] = 7
            if i == at and kind == "three_alleles":
                gt, k = [v + [E] for v in gt], 3
                gt[1] = [gc.gt_value(0), gc.gt_value(1), gc.gt_value(1)]
            if i == at and kind == "gq_128":
                gq[1], gq_t = [128], 2
            return [("GT", t, k, gt)] + ([("PL", 2, len(pl[0]), pl)] if mode == 8 else [("GQ", gq_t, 1, gq)])
        name = "f%d" % at
        samples, trecs, crecs = gc.simple_pair(tmp_path, name, 9, 7, 20 + at, fields, nal=3, alleles=(lambda i: al17) if kind.endswith("allele_sixteen") else None,
                                               ids=lambda i: "r" * (5 * i % 16))
        if kind in ("truth_allele_sixteen", "both_allele_sixteen"):
            trecs[at].fields[0][3][2] = [gc.gt_value(16), gc.gt_value(1)]     # the truth record's third sample: allele 16 is AT, a base
        p = gc.Pair(tmp_path, name, samples, trecs, crecs, has_gq=mode != 8, has_pl=mode == 8)
        kw = dict(do_gq=mode, per_site=True, batch_records=7)
        want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
        got = resident(tmp_path, p.t_bgzf, p.c_bgzf, bcf_direct=True, **kw)
        got.same(want)
        assert p.not_plain(mode) == (1, 7) and want.rc == (1 if kind in BCF_ODD_STOPS else 0), want.text[-1000:]
        if want.rc == 0:
            assert (got.records, got.redone) == (7, 1)
        else:
            assert want.stdout.count("\n") == at * 9 + BCF_ODD_STOPS[kind]   # the records before it (PL is read before any sample is listed)


def test_a_bcf_record_whose_line_stands_as_text(tmp_path):
    """a tab inside an allele name: the record's nine columns would not stand where a reader of the line looks, so its whole line is
    written from the record's bytes, copied down from the resident file, and the run stops there as --on-device 0 stops on the file"""
    def fields(rnd, i, tg, nal):
        return [("GT", 1, 2, [[gc.gt_value(a), gc.gt_value(b)] for a, b in tg]), ("GQ", 1, 1, [[rnd.randint(1, 127)] for _ in tg])]
    for side in ("truth", "call"):
        al = lambda i: ["A", "C", "G\tG" if i == 4 else "G", "T"]
        samples, trecs, crecs = gc.simple_pair(tmp_path, "tab", 9, 7, 5, fields, alleles=al)
        if side == "truth":
            crecs[4].alleles = ["A", "C", "G", "T"]
        else:
            trecs[4].alleles = ["A", "C", "G", "T"]
        tb = bgz(tmp_path, "t.bcf.gz", gc.bcf_bytes(samples, trecs, False, False), 300)
        cb = bgz(tmp_path, "c.bcf.gz", gc.bcf_bytes(samples, crecs, True, False), 300)
        kw = dict(do_gq=2, per_site=True, batch_records=3, bcf_direct=True)
        want = host(tmp_path, tb, cb, **kw)
        got = resident(tmp_path, tb, cb, **kw)
        got.same(want)
        assert want.rc == 1 and want.stdout.count("\n") == 4 * 9, want.text[-1000:]
        staged(tmp_path, tb, cb, **kw).same(want)


# ---- stops ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["truth_missing", "no_gq", "no_truth_site"])
def test_a_stop_at_each_place(kind, tmp_path):
    n, pos = 5, list(range(20, 29))
    for at in (0, 4, 8):                                                    # the first, a middle and the last record (batches of 4)
        tl = [line(q, n, False) for q in [19] + pos + [40]]
        cl = [line(q, n, True) for q in pos]
        if kind == "truth_missing":
            f = tl[1 + at].split("\t"); f[9 + n - 1] = "./1"; tl[1 + at] = "\t".join(f)
        elif kind == "no_gq":
            f = cl[at].split("\t"); f[8] = "GT"; f[9:] = [x.split(":")[0] for x in f[9:]]; cl[at] = "\t".join(f)
        else:
            del tl[1 + at]
        body = "\n".join(HEAD + [names_line(n)]) + "\n"
        tz = bgz(tmp_path, "t%d.vcf.gz" % at, (body + "\n".join(tl) + "\n").encode(), 500)
        cz = bgz(tmp_path, "c%d.vcf.gz" % at, (body + "\n".join(cl) + "\n").encode(), 500)
        kw = dict(do_gq=6 if kind == "no_gq" else 2, per_site=True, batch_records=4)
        want = host(tmp_path, tz, cz, **kw)
        got = resident(tmp_path, tz, cz, **kw)
        got.same(want)
        assert want.rc == 1 and {"truth_missing": "the true genotype is missing", "no_gq": "has no GQ tag", "no_truth_site": "the truth file has none"}[kind] in want.text
        assert want.stdout.count("\n") == at * n + (n - 1 if kind == "truth_missing" else 0)
        # the same records as BCF (a truth site the call file lacks and a record without GQ are what the heads say, too)
        _, trecs = gc.from_text(write(tmp_path / "t.vcf", (body + "\n".join(tl) + "\n").encode()))
        samples, crecs = gc.from_text(write(tmp_path / "c.vcf", (body + "\n".join(cl) + "\n").encode()))
        tb = bgz(tmp_path, "t%d.bcf.gz" % at, gc.bcf_bytes(samples, trecs, False, False), 500)
        cb = bgz(tmp_path, "c%d.bcf.gz" % at, gc.bcf_bytes(samples, crecs, True, False), 500)
        resident(tmp_path, tb, cb, bcf_direct=True, **kw).same(want)


# ---- fallbacks ------------------------------------------------------------------------------------------------------------------------
def test_files_that_cannot_be_resident_say_why(odd_pair, tmp_path):
    p = odd_pair
    kw = dict(do_gq=2, per_site=True, batch_records=16)
    want = host(tmp_path, p.t_vcf, p.c_vcf, **kw)
    nonplain = p.not_plain(2)[0]
    tt, ct = bgz(tmp_path, "t.vcf.gz", p.t_vcf), bgz(tmp_path, "c.vcf.gz", p.c_vcf)
    gz = lambda name, src: write(tmp_path / name, gzip.compress(open(src, "rb").read()))
    cases = [(p.t_vcf, p.c_vcf, {}, "not a series of BGZF members"),                                   # plain text
             (gz("t.gz", p.t_vcf), gz("c.gz", p.c_vcf), {}, "not a series of BGZF members"),          # gzip that is not BGZF
             (gz("t.bcf.gz", p.t_bcf), p.c_bcf, dict(bcf_direct=True), "not a series of BGZF members"),   # BCF in gzip, raw BCF
             (tt, ct, dict(resident_max_bytes=0), "exceed what --resident-max-bytes leaves"),
             (p.t_bgzf, p.c_bgzf, dict(bcf_direct=False), "the file is BCF and --bcf-direct is 0")]
    for t, c, extra, why in cases:
        got = resident(tmp_path, t, c, both=False, **dict(kw, **extra))
        got.same(want)
        assert [i["resident"] for i in got.inputs] == [0, 0] and all(why in i["why"] for i in got.inputs), got.raw[-2000:]
        assert (got.records, got.redone) == (60, nonplain) and got.text_up + got.vec_up > 0


def test_a_record_the_walk_refuses_hands_the_file_back(tmp_path):
    """a call record whose sample count is not the header's: rb::Why names it, the host reader reads the file and stops where it stops"""
    def fields(rnd, i, tg, nal):
        return [("GT", 1, 2, [[gc.gt_value(a), gc.gt_value(b)] for a, b in tg]), ("GQ", 1, 1, [[rnd.randint(1, 127)] for _ in tg])]
    samples, trecs, crecs = gc.simple_pair(tmp_path, "ns", 5, 6, 31, fields)
    good = gc.bcf_bytes(samples, crecs, True, False)
    upto = len(gc.bcf_bytes(samples, crecs[:3], True, False))
    bad = bytearray(good)
    assert bad[upto + 8 + 20] == 5
    bad[upto + 8 + 20] = 4                                                  # n_sample of the fourth record
    p = gc.Pair(tmp_path, "ns", samples, trecs, crecs, has_pl=False)
    cb = bgz(tmp_path, "bad.bcf.gz", bytes(bad))
    kw = dict(do_gq=6, per_site=True, bcf_direct=True)
    want = host(tmp_path, p.t_bgzf, cb, **kw)
    got = resident(tmp_path, p.t_bgzf, cb, both=False, **kw)
    got.same(want)
    assert want.rc == 1 and "has 4 samples, the header names 5 samples" in want.text
    assert [i["resident"] for i in got.inputs] == [1, 0] and "record 4: a sample count other than the header's" in got.inputs[1]["why"]


# ---- golden ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth,call,mode,ref", [("truth.vcf", "call.vcf", 0, "test_doGq0.tsv"), ("truth3.vcf", "call3.vcf", 7, "test3_doGq7.tsv"),
                                                 ("truth3.vcf", "call3_nogq_withpl.vcf", 8, "test3_doGq7.tsv")])
def test_the_references_pairs_as_bgzf(truth, call, mode, ref, tmp_path):
    t, c = os.path.join(GOLD, "data", truth), os.path.join(GOLD, "data", call)
    got = resident(tmp_path, bgz(tmp_path, "t.vcf.gz", t, 300), bgz(tmp_path, "c.vcf.gz", c, 300), do_gq=mode)
    assert got.rc == 0 and got.out == open(os.path.join(GOLD, "reference", ref), "rb").read() and got.redone == 0, got.raw[-2000:]
    got.same(host(tmp_path, t, c, do_gq=mode))
