"""setalleles_hip --resident 1 (vcfgl_amd/csrc/misc/setalres.hip, salres_core.h: a BGZF file of BCF stays in GPU memory, the vectors are
relabelled where the inflater wrote them, the output records are assembled and -- for -O b -- compressed on the GPU): every byte the
flag writes -- the output file (the decompressed stream for -O b), stderr without the [setalleles] and [input] lines, the return code --
equals what --on-device 0 writes (which tests/test_setalhip_cli_cpu.py holds against the model), every record was assembled on the
device and no batch was handed back, so the flag has really done the work.  Also: the conditions on the input that make the byte
gather meet every alignment (asserted on the CPU, fixed by seed), a record of each PL width, vectors shorter than the old genotype
count, records without a touched field and without FORMAT, a PL overflow at the first, a middle and the last record of a batch (the
batch is handed back and the host path stops the run), the files that cannot be resident, and the tie to the simulator.
Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

import bcf_reader
import fgl_file_model as ff
import sal_file_model as M
from vcfgl_amd import setalleles as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 120
BREC_BYTES, DESC_BYTES = 64, 120       # sizeof(sal::BRec), sizeof(salres::Desc): what goes up per record beside its new shared block
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started


def _device(path, tsv, prefix, mode, **kw):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        rc, so, se = S.set_file(path, tsv, prefix, mode, on_device=True, device_inflate=True, resident=True, verbose=True, timeout=TIMEOUT, **kw)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("setalleles_hip ran out of time: no further GPU process is started")
    if rc in (-6, -11, 134, 139, 124, 137):
        _gave_up.append("setalleles_hip")
        pytest.fail("setalleles_hip ended with status %d: no further GPU process is started" % rc)
    return rc, so, se


def _host(path, tsv, prefix, mode="u"):
    return S.set_file(path, tsv, prefix, mode, on_device=False, verbose=True, timeout=TIMEOUT)


def _plain(stderr, prefix):
    return "".join(ln for ln in stderr.splitlines(True) if not ln.startswith(("[setalleles]", "[input]"))).replace(prefix, "PREFIX")


def _stream(prefix):
    """the output file's decompressed stream; a BGZF file has every member's header, CRC and size and the EOF member checked"""
    fn = prefix + ".bcf"
    if not os.path.exists(fn):
        return None
    raw = open(fn, "rb").read()
    return b"".join(bcf_reader.bgzf_blocks(raw)) if raw[:2] == b"\x1f\x8b" else raw


def _line(stderr):
    m = re.search(r"\[setalleles\] on-device 1: records (\d+), redone on the host (\d+), bytes sent up (\d+), received (\d+);.*; resident (\d): assembled on the device (\d+), "
                  r"batches handed back (\d+), (member|record) bytes received (\d+); relabel", stderr)
    assert m, stderr[-2000:]
    return dict(zip(("records", "redone", "up", "down", "resident", "assembled", "back", "kind", "made"), [int(g) if g.isdigit() else g for g in m.groups()]))


def bgzf(data, block):
    """fgl_file_model.bgzf in linear time (a file of 997-byte members has thousands of them)"""
    parts = []
    for at in list(range(0, len(data), block)) + [len(data)]:
        chunk = data[at:at + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(chunk) + z.flush()
        parts += [b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00", struct.pack("<H", len(body) + 25), body, struct.pack("<II", zlib.crc32(chunk), len(chunk))]
    return b"".join(parts)


def test_the_linear_bgzf_writer_is_the_models():
    data = bytes(range(256)) * 40
    assert bgzf(data, 997) == ff.bgzf(data, 997) and bgzf(b"", 60000) == ff.bgzf(b"", 60000)


def _shared_bytes(stream):
    """the sum of l_shared over the records of a BCF stream"""
    off, total = 9 + struct.unpack_from("<I", stream, 5)[0], 0
    while off < len(stream):
        ls, li = struct.unpack_from("<II", stream, off)
        total += ls
        off += 8 + ls + li
    return total


def _same(tmp_path, path, tsv, mode, host, n_records, **kw):
    """--resident 1 on one file against the host's (rc, plain stderr, stream, stderr): equal, all on the device, what went up is the
    compressed file and the descriptors"""
    pd = str(tmp_path / "dev")
    rd = _device(path, tsv, pd, mode, **kw)
    assert rd[0] == host[0], (rd[2][-2000:], host[3][-2000:])
    assert _plain(rd[2], pd) == host[1]
    got = _stream(pd)
    assert got == host[2]
    raw = open(pd + ".bcf", "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == (mode == "b")
    inp = [ln for ln in rd[2].splitlines() if ln.startswith("[input]")]
    assert len(inp) == 1 and ": resident 1, members " in inp[0] and "device-inflate" not in inp[0], inp
    c = _line(rd[2])
    assert (c["records"], c["redone"], c["resident"], c["assembled"], c["back"]) == (n_records, 0, 1, n_records, 0), c
    assert c["kind"] == ("member" if mode == "b" else "record") and (c["made"] > 0) == (n_records > 0)
    if mode == "u":
        assert c["made"] == len(got) - (9 + struct.unpack_from("<I", got, 5)[0])
    assert c["up"] == os.path.getsize(path) + n_records * (BREC_BYTES + DESC_BYTES) + _shared_bytes(got), c
    return rd


def _write(dirname, name, brecs, recs, n_samples, block=60000):
    path, tsv = str(dirname / (name + ".bcf.gz")), str(dirname / (name + ".tsv"))
    with open(path, "wb") as f:
        f.write(bgzf(M.encode_bcf(brecs, n_samples), block))
    open(tsv, "w").write(M.tsv_text(recs))
    return path, tsv


def _host_of(dirname, name, path, tsv):
    ph = str(dirname / (name + "_host"))
    rh = _host(path, tsv, ph)
    return rh[0], _plain(rh[2], ph), _stream(ph), rh[2]


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("salres_shapes")


_files = {}


def _shape(shapes_dir, N, R):
    """the generated records of a shape, their encoded bytes and the host's output: made once"""
    if (N, R) not in _files:
        recs = M.make_records(N, R, seed=2000 * N + R, wide_pl=True)
        brecs = M.bcf_records(recs, N, end_every=5)
        data = M.encode_bcf(brecs, N)
        tsv = str(shapes_dir / ("n%d_r%d.tsv" % (N, R)))
        open(tsv, "w").write(M.tsv_text(recs))
        path = str(shapes_dir / ("n%d_r%d_60000.bcf.gz" % (N, R)))
        open(path, "wb").write(bgzf(data, 60000))
        _files[(N, R)] = (data, tsv, _host_of(shapes_dir, "n%d_r%d" % (N, R), path, tsv))
    return _files[(N, R)]


def _member_file(shapes_dir, N, R, block):
    data, tsv, host = _shape(shapes_dir, N, R)
    path = str(shapes_dir / ("n%d_r%d_%d.bcf.gz" % (N, R, block)))
    if not os.path.exists(path):
        open(path, "wb").write(bgzf(data, block))
    return path, tsv, host


# ---- the conditions on the input: asserted on the CPU, fixed by the seeds above -----------------------------------------------------
def _typed(b, o):
    t, n = b[o] & 15, b[o] >> 4
    if n < 15:
        return t, n, o + 1
    w = {1: 1, 2: 2, 3: 4}[b[o + 1] & 15]
    return t, int.from_bytes(b[o + 2:o + 2 + w], "little"), o + 2 + w


_WIDTH = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}


def _fields(stream, N):
    """per record of a BCF stream: (where it begins, [(key, field at, data at, field end)])"""
    off, out = 9 + struct.unpack_from("<I", stream, 5)[0], []
    while off < len(stream):
        ls, li = struct.unpack_from("<II", stream, off)
        n_fmt = stream[off + 8 + 23]
        p, fields = off + 8 + ls, []
        for _ in range(n_fmt):
            at = p
            t, n, p = _typed(stream, p)
            key = int.from_bytes(stream[p:p + _WIDTH[t]], "little")
            p += _WIDTH[t] * n
            t, n, p = _typed(stream, p)
            fields.append((key, at, p, p + _WIDTH[t] * n * N))
            p = fields[-1][3]
        assert p == off + 8 + ls + li
        out.append((off, fields))
        off = p
    return out


def test_the_inputs_meet_every_alignment(shapes_dir):
    """the vector blocks begin at all four residues mod 4, the copy runs' sources and the records' places in the assembled batch cover
    all 16 residues mod 16, and a copy run is shorter than 16 bytes"""
    touched = {M.BCF_DICT[t] for t in M.TAGS}
    data, tsv, host = _shape(shapes_dir, 63, 300)
    block_res, run_res, short = set(), set(), False
    for off, fields in _fields(data, 63):
        run_at = None                                                  # where the copy run that is open begins
        for key, at, data_at, end in fields:
            if key in touched:
                block_res.add(data_at % 4)
                if run_at is not None:
                    run_res.add(run_at % 16)
                run_at = None
            elif run_at is None:
                run_at = at
        if run_at is not None:
            run_res.add(run_at % 16)
    assert block_res == {0, 1, 2, 3} and run_res == set(range(16))
    first = 9 + struct.unpack_from("<I", host[2], 5)[0]
    assert {(off - first) % 16 for off, _ in _fields(host[2], 63)} == set(range(16))           # --batch-records 4096: one batch
    data1, _, _ = _shape(shapes_dir, 1, 7)
    for off, fields in _fields(data1, 1):
        short = short or (fields[0][0] == M.BCF_DICT["DP"] and fields[0][3] - fields[0][1] < 16)   # N = 1, one int8 DP: key, descriptor, a byte
    assert short


# ---- equality with the host path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["b", "u"])
@pytest.mark.parametrize("block", [60000, 4096, 997])
@pytest.mark.parametrize("batch", [1, 7, 4096])
@pytest.mark.parametrize("R", [1, 7, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_wavefront_workgroup_batch_and_member_boundaries(tmp_path, shapes_dir, N, R, batch, block, mode):
    path, tsv, host = _member_file(shapes_dir, N, R, block)
    assert host[0] == 0, host[3][-2000:]
    _same(tmp_path, path, tsv, mode, host, R, batch_records=batch)


@pytest.mark.parametrize("n_old,n_new", [(o, n) for o in range(2, 6) for n in range(2, o + 1)])
def test_every_pair_of_allele_counts(tmp_path, n_old, n_new):
    recs = M.make_records(67, 9, seed=60 + 10 * n_old + n_new, n_old=n_old, n_new=n_new)
    brecs = M.bcf_records(recs, 67, end_every=5)
    path, tsv = _write(tmp_path, "in", brecs, recs, 67)
    host = _host_of(tmp_path, "in", path, tsv)
    _same(tmp_path, path, tsv, "b" if (n_old + n_new) % 2 else "u", host, 9, batch_records=4)
    assert host[0] == 0 and M.read_bcf(str(tmp_path / "dev.bcf"))[1] == M.run_bcf(brecs, [r["target"] for r in recs]).records


@pytest.mark.parametrize("tags", M.TAG_SETS)
@pytest.mark.parametrize("qs", [False, True])
def test_every_tag_set(tmp_path, tags, qs):
    recs = M.make_records(67, 9, seed=9, tags=tags, qs=qs)
    brecs = M.bcf_records(recs, 67, end_every=5)
    path, tsv = _write(tmp_path, "in", brecs, recs, 67, block=4096)
    host = _host_of(tmp_path, "in", path, tsv)
    _same(tmp_path, path, tsv, "u" if qs else "b", host, 9, batch_records=4)
    assert host[0] == 0 and M.read_bcf(str(tmp_path / "dev.bcf"))[1] == M.run_bcf(brecs, [r["target"] for r in recs]).records


def test_a_record_of_each_pl_width_and_a_batch_that_mixes_them(tmp_path):
    recs = M.make_records(70, 12, seed=31, tags="GL:PL", wide_pl=True)
    brecs = M.bcf_records(recs, 70)
    path, tsv = _write(tmp_path, "in", brecs, recs, 70)
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    widths = [t for r in want.records for k, t, per in r["fmt"] if k == "PL"]
    assert want.stop is None and set(widths) == {1, 2, 3} and len(set(widths[:4])) > 1       # (one batch of 12 holds all three)
    host = _host_of(tmp_path, "in", path, tsv)
    for batch, mode in ((1, "u"), (4096, "u"), (4096, "b")):
        _same(tmp_path, path, tsv, mode, host, 12, batch_records=batch)
        body, got = M.read_bcf(str(tmp_path / "dev.bcf"))
        assert got == want.records and body == b"".join(M.encode_record(r, 70) for r in want.records)


def test_short_vectors_and_records_without_a_touched_field_or_format(tmp_path):
    """vectors shorter than the old genotype count (end-of-vector fills them), a record none of whose fields is touched, one with no FORMAT"""
    recs = M.make_records(66, 10, seed=44, n_old=4, n_new=3)
    brecs = M.bcf_records(recs, 66, end_every=3)
    for i in (1, 4, 8):
        brecs[i]["fmt"] = [(k, t, [v[:2 + i % 3] for v in per]) if k in ("GL", "GP") else (k, t, per) for k, t, per in brecs[i]["fmt"]]
    brecs[2]["fmt"] = [(k, t, per) for k, t, per in brecs[2]["fmt"] if k not in M.TAGS]
    brecs[6]["fmt"] = []
    path, tsv = _write(tmp_path, "in", brecs, recs, 66, block=997)
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    assert want.stop is None and any(len(per[0]) == 3 for k, t, per in brecs[4]["fmt"] if k == "GL")       # (of 10 old genotypes)
    host = _host_of(tmp_path, "in", path, tsv)
    for batch, mode in ((3, "b"), (4096, "u")):
        _same(tmp_path, path, tsv, mode, host, 10, batch_records=batch)
        assert host[0] == 0 and M.read_bcf(str(tmp_path / "dev.bcf"))[1] == want.records


# ---- stops --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [7, 10, 13])
@pytest.mark.parametrize("mode", ["b", "u"])
def test_a_pl_overflow_at_the_first_a_middle_and_the_last_record_of_a_batch(tmp_path, at, mode):
    recs = M.make_records(5, 21, seed=78, tags="GL:PL", n_old=3, n_new=2)
    brecs = M.bcf_records(recs, 5)
    k = next(i for i, (key, t, per) in enumerate(brecs[at]["fmt"]) if key == "PL")
    hom_het = [-2000000000, 2000000000, -2000000000, 2000000000, 2000000000, -2000000000]      # any pair of alleles overflows
    brecs[at]["fmt"][k] = ("PL", 3, [list(hom_het) if s == 3 else [0, 1, 2, 3, 4, 5] for s in range(5)])
    path, tsv = _write(tmp_path, "in", brecs, recs, 5)
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    host = _host_of(tmp_path, "in", path, tsv)
    assert want.stop == ("pl", recs[at]["pos"]) and len(want.records) == at
    assert host[0] == 1 and "Sample 3 at position %d" % recs[at]["pos"] in host[1]
    pd = str(tmp_path / "dev")
    rd = _device(path, tsv, pd, mode, batch_records=7)
    assert rd[0] == 1 and _plain(rd[2], pd) == host[1] and "finished" not in rd[2]
    assert _stream(pd) == host[2] and M.read_bcf(pd + ".bcf")[1] == want.records
    c = _line(rd[2])                                                   # the batch of the stop came back whole; the batches before it were the device's
    assert (c["resident"], c["back"], c["redone"], c["assembled"]) == (1, 1, 0, 7 * (at // 7)), c


# ---- files that cannot be resident ----------------------------------------------------------------------------------------------------
def _not_resident(tmp_path, path, tsv, host, word, **kw):
    pd = str(tmp_path / "dev")
    rd = _device(path, tsv, pd, "u", **kw)
    assert rd[0] == host[0] == 0 and _plain(rd[2], pd) == host[1] and _stream(pd) == host[2]
    inp = [ln for ln in rd[2].splitlines() if ln.startswith("[input]")]
    assert inp and ": resident 0 (" in inp[0] and word in inp[0], inp
    c = _line(rd[2])
    assert (c["resident"], c["assembled"], c["back"], c["redone"]) == (0, 0, 0, 0)


def test_files_that_cannot_be_resident_run_as_resident_0(tmp_path):
    recs = M.make_records(9, 14, seed=3, n_old=5, n_new=3)
    brecs = M.bcf_records(recs, 9, end_every=5)
    data = M.encode_bcf(brecs, 9)
    tsv = str(tmp_path / "in.tsv")
    open(tsv, "w").write(M.tsv_text(recs))
    raw, gz, bgz, odd = (str(tmp_path / n) for n in ("raw.bcf", "plain.bcf.gz", "in.bcf.gz", "odd.bcf.gz"))
    open(raw, "wb").write(data)
    open(gz, "wb").write(gzip.compress(data, 6))
    open(bgz, "wb").write(bgzf(data, 4096))
    host = _host_of(tmp_path, "in", bgz, tsv)
    _not_resident(tmp_path, raw, tsv, host, "the file is not a series of BGZF members")
    _not_resident(tmp_path, gz, tsv, host, "the file is not a series of BGZF members")
    _not_resident(tmp_path, bgz, tsv, host, "exceed --resident-max-bytes", resident_max_bytes=1)
    # a FORMAT descriptor the host reads and rb_core.h does not know: fifteen GLs counted by a vector of two int8, the first of which counts
    rec = M.encode_record(brecs[5], 9)
    gl = bytes([0x11, M.BCF_DICT["GL"], 0xF5, 0x11, 0x0F])
    assert rec.count(gl) == 1
    ls, li = struct.unpack_from("<II", rec, 0)
    rec = struct.pack("<II", ls, li + 1) + rec[8:].replace(gl, gl[:3] + bytes([0x21, 0x0F, 0x00]))
    body = b"".join(rec if i == 5 else M.encode_record(r, 9) for i, r in enumerate(brecs))
    open(odd, "wb").write(bgzf(M.bcf_header_bytes(9) + body, 4096))
    host_odd = _host_of(tmp_path, "odd", odd, tsv)
    assert host_odd[0] == 0 and host_odd[2] == host[2]
    _not_resident(tmp_path, odd, tsv, host_odd, "record 6: a typed descriptor outside the walk's rules")


# ---- the tie to the simulator ---------------------------------------------------------------------------------------------------------
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data", "data3.vcf")
SIM = ["--seed", "42", "-e", "0.05", "-d", "3", "-explode", "1", "-doUnobserved", "4", "-addPL", "1", "-addGP", "1", "-addQS", "1", "-O", "b"]


def test_tie_to_the_simulator(tmp_path):
    """--resident 1 -O b on the -O b file of a plain vcfgl_hip run equals --resident 0 on it, decompressed"""
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    plain, tsv = str(tmp_path / "plain"), str(tmp_path / "a.tsv")
    try:
        r = subprocess.run([VCFGL, "-i", DATA3, "-o", plain] + SIM, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("vcfgl_hip ran out of time: no further GPU process is started")
    if r.returncode in (-6, -11, 134, 139, 124, 137):
        _gave_up.append("vcfgl_hip")
        pytest.fail("vcfgl_hip ended with status %d: no further GPU process is started" % r.returncode)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = list(bcf_reader.Reader(plain + ".bcf").records())
    assert len(recs) >= 5 and all(len(r["alleles"]) == 5 for r in recs)
    with open(tsv, "w") as f:
        for i, r in enumerate(recs):
            t = (r["alleles"][i % 5:] + r["alleles"][:i % 5])[:2 + i % 4]
            f.write(t[0] + "\t" + ",".join(t[1:]) + "\n")
    p0 = str(tmp_path / "res0")
    r0 = S.set_file(plain + ".bcf", tsv, p0, "b", on_device=True, device_inflate=True, resident=False, verbose=True, timeout=TIMEOUT)
    assert r0[0] == 0, r0[2][-2000:]
    host = (0, _plain(r0[2], p0), _stream(p0), r0[2])
    _same(tmp_path, plain + ".bcf", tsv, "b", host, len(recs))
