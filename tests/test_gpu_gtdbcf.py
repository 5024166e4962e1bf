"""gtdiscordance_hip --on-device 1 --bcf-direct 1 on the device (k_gtd_bcf_decode of vcfgl_amd/csrc/misc/gtdisc.hip): every byte it
writes is what --on-device 1 --bcf-direct 0 writes from the text of the same BCF records -- on shapes that put sample, record and
batch boundaries everywhere, at every width of GT / GQ / PL, with the vectors at every file offset mod 4, on mixed pairs, on BGZF
inflated on the device, with records handed back to the host at the first, a middle and the last place of a batch, and with a stop
inside a batch.  The model (tests/gtdisc_model.py on the rendered text) says on the CPU how many records are not plain; the [bcf]
line must report exactly that many redone.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os
import re
import subprocess

import pytest

import gtdbcf_cases as gc
import gtdisc_model as gm
from vcfgl_amd import discordance as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data", "data3.vcf")
TIMEOUT = 120
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started
E, M = gc.E, gc.M


def _check_alive(rc, what):
    if rc in (-6, -11, 134, 139, 124, 137):
        _gave_up.append(what)
        pytest.fail("%s ended with status %d: no further GPU process is started" % (what, rc))


def _device(truth, call, out, **kw):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    if os.path.exists(out):
        os.remove(out)
    try:
        rc, so, se = D.compare_files(truth, call, out, on_device=True, verbose=True, timeout=TIMEOUT, **kw)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("gtdiscordance_hip ran out of time: no further GPU process is started")
    _check_alive(rc, "gtdiscordance_hip")
    text = "".join(ln for ln in se.splitlines(True) if not ln.startswith(("[gtdisc]", "[bcf]", "[input]"))).replace(out, "OUT")
    text = re.sub(r"truth file \S+ and the call file \S+", "truth file T and the call file C", text)
    return rc, open(out, "rb").read() if os.path.exists(out) else None, so, text, _bcf_line(se)


def _bcf_line(stderr):
    m = re.search(r"\[bcf\] bcf-direct 1: records judged from their vectors: truth (\d+), call (\d+); redone on the host (\d+); "
                  r"vector bytes sent up (\d+), text bytes sent up (\d+); device stage ([0-9.]+) ms over (\d+) batches", stderr)
    return None if m is None else tuple(int(m.group(k)) for k in (1, 2, 3, 4, 5))


def _same(tmp_path, truth, call, want=None, **kw):
    """--bcf-direct 1 against --bcf-direct 0 (or a result of it computed before): status, output file, stdout and messages"""
    inflate = kw.pop("device_inflate", None)
    if want is None:
        want = _device(truth, call, str(tmp_path / "text.tsv"), bcf_direct=False, **kw)
    got = _device(truth, call, str(tmp_path / "direct.tsv"), bcf_direct=True, device_inflate=inflate, **kw)
    assert got[0] == want[0], (got[3][-1500:], want[3][-1500:])
    assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
    return got


# ---- boundaries -----------------------------------------------------------------------------------------------------------------------
SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]
MODES = [dict(do_gq=6), dict(do_gq=2, per_site=True)]
_shape_cache = {}


def _shape(tmp_path_factory, k):
    """the pair of shape k and what --on-device 1 --bcf-direct 0 gives for it under each mode: made once"""
    if k not in _shape_cache:
        n, r = SHAPES[k]
        d = tmp_path_factory.mktemp("gtdbcf_shape%d" % k)
        p = gc.pair_from_generator(d, "s", n, r, "GT:GQ", seed=4000 + k, first_pos=(8 if k % 2 else 2 ** 31 - 1000))
        assert all(p.not_plain(m["do_gq"]) == (0, r) for m in MODES)         # all plain, says the model: nothing may be handed back
        _shape_cache[k] = (p, [_device(p.t_bcf, p.c_bcf, str(d / ("want%d.tsv" % j)), bcf_direct=False, **m) for j, m in enumerate(MODES)])
    return _shape_cache[k]


@pytest.mark.parametrize("batch", [1, 7, 4096])
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_boundaries_of_samples_records_and_batches(k, batch, tmp_path, tmp_path_factory):
    p, want = _shape(tmp_path_factory, k)
    n, r = SHAPES[k]
    for m, w in zip(MODES, want):
        assert w[0] == 0, w[3][-1500:]
        got = _same(tmp_path, p.t_bcf, p.c_bcf, want=w, batch_records=batch, **m)
        direct_t, direct_c, redone, vec_up, text_up = got[4]
        assert (direct_t, direct_c, redone, text_up) == (r, r, 0, 0) and vec_up > 0
        assert len(got[1]) > 0


# ---- types and shapes -----------------------------------------------------------------------------------------------------------------
def _gt_fields(t, n_val, gq_t=1, host_at=None):
    def fields(rnd, i, tg, nal):
        gt = [[gc.gt_value(a), gc.gt_value(b, rnd.randrange(2))] + [E] * (n_val - 2) for a, b in tg]
        for v in gt:
            if rnd.random() < 0.1:
                v[rnd.randrange(2)] = rnd.choice((M, gc.gt_value(-1)))
        if host_at == i:
            gt[len(gt) // 2] = [gc.gt_value(0), gc.gt_value(1), gc.gt_value(1)]     # three real alleles: the host reader's, which stops
        return [("GT", t, n_val, gt), ("DP", 1, 1, [[rnd.randrange(100)] for _ in tg]), ("GQ", gq_t, 1, [[rnd.choice((1, 9, 10, 99, 100, 127))] for _ in tg])]
    return fields


@pytest.mark.parametrize("n_val", [2, 3])
@pytest.mark.parametrize("t", [1, 2, 3])
def test_gt_and_gq_at_every_width(t, n_val, tmp_path):
    samples, trecs, crecs = gc.simple_pair(tmp_path, "w", 67, 9, 100 + 10 * t + n_val, _gt_fields(t, n_val, gq_t=(t % 3) + 1), truth_type=(t + n_val) % 3 + 1)
    p = gc.Pair(tmp_path, "w", samples, trecs, crecs, has_pl=False)
    for m in MODES:
        got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=4, **m)
        assert got[0] == 0 and got[4][:3] == (9, 9, 0) and p.not_plain(m["do_gq"]) == (0, 9)


def test_three_real_alleles_go_to_the_host_reader(tmp_path):
    samples, trecs, crecs = gc.simple_pair(tmp_path, "h", 67, 9, 7, _gt_fields(1, 3, host_at=5))
    p = gc.Pair(tmp_path, "h", samples, trecs, crecs, has_pl=False)
    got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=4, do_gq=2, per_site=True)
    res = gm.compare(p.t_vcf, p.c_vcf, 2, per_site=True)
    assert got[0] == 1 and res.stop.pos == 6 and got[1].decode() == "".join(res.listing) and got[2] == "".join(res.per_site)


def _pl_fields(pl_t, flaw=None):
    def fields(rnd, i, tg, nal):
        nG = nal * (nal + 1) // 2
        gt, pl = [], []
        for s, (a, b) in enumerate(tg):
            missing = rnd.random() < 0.15
            gt.append([gc.gt_value(-1), gc.gt_value(-1)] if missing else [gc.gt_value(a), gc.gt_value(b, 1)])
            v = [rnd.choice((3, 17, 60, 126, 0)) if pl_t == 1 else rnd.choice((3, 17, 126, 127, 128, 255, 1000, 9999, 0)) for _ in range(nG)]
            v[rnd.randrange(nG)] = M if rnd.random() < 0.2 else 0
            if flaw == i and s == len(tg) - 1:
                v = [5] * nG                                           # no zero found: the host reader's, which stops
            pl.append(v)
        return [("GT", 1, 2, gt), ("PL", pl_t, nG, pl)]
    return fields


@pytest.mark.parametrize("pl_t", [1, 2])
@pytest.mark.parametrize("nal", [1, 2, 3, 4, 5])
def test_doGQ_8_reads_pl_of_one_to_five_alleles(nal, pl_t, tmp_path):
    samples, trecs, crecs = gc.simple_pair(tmp_path, "pl", 66, 6, 50 + nal, _pl_fields(pl_t), nal=nal)
    p = gc.Pair(tmp_path, "pl", samples, trecs, crecs, has_gq=False)
    got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=4, do_gq=8, per_site=True)
    assert got[0] == 0 and got[4][:3] == (6, 6, 0) and p.not_plain(8) == (0, 6), got[3][-1500:]
    assert got[4][3] == 66 * 2 * 12 + (66 * 6 * pl_t * nal * (nal + 1) // 2 if nal > 1 else 0)         # PL goes up only where it is read


def test_doGQ_8_without_a_zero_stops_as_the_text_route(tmp_path):
    samples, trecs, crecs = gc.simple_pair(tmp_path, "nz", 66, 6, 9, _pl_fields(2, flaw=3), nal=3)
    p = gc.Pair(tmp_path, "nz", samples, trecs, crecs, has_gq=False)
    got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=4, do_gq=8, per_site=True)
    assert got[0] == 1 and "no PL value is 0 or missing" in got[3] and len(got[2]) > 0


def test_vectors_at_every_file_offset_mod_4(tmp_path):
    ids = lambda i: "r" * (1 + i % 4)
    alleles = lambda i: ["A" * (1 + (i // 4) % 3), "C", "G" * (1 + i % 2)]
    samples, trecs, crecs = gc.simple_pair(tmp_path, "o", 65, 12, 3, _gt_fields(1, 2), nal=3, ids=ids, alleles=alleles)
    p = gc.Pair(tmp_path, "o", samples, trecs, crecs, has_pl=False)
    assert {x % 4 for x in gc.vector_offsets(samples, crecs, "GT", True, False)} == {0, 1, 2, 3}
    assert {x % 4 for x in gc.vector_offsets(samples, crecs, "GQ", True, False)} == {0, 1, 2, 3}
    assert {x % 4 for x in gc.vector_offsets(samples, trecs, "GT", False, False)} == {0, 1, 2, 3}
    for m in MODES:
        got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=5, **m)
        assert got[0] == 0 and got[4][:3] == (12, 12, 0)


# ---- mixed pairs, BGZF ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtdbcf_odd")
    return gc.pair_from_generator(d, "m", 65, 60, "GT:PL:GQ", seed=11, odd_share=0.1)


def test_mixed_pairs_in_both_orders(odd_pair, tmp_path):
    p = odd_pair
    for m in (dict(do_gq=2, per_site=True), dict(do_gq=8)):
        want = _device(p.t_vcf, p.c_vcf, str(tmp_path / "want.tsv"), bcf_direct=False, batch_records=16, **m)
        nonplain = p.not_plain(m["do_gq"])[0]
        assert want[0] == 0 and nonplain > 0
        for t, c in ((p.t_bcf, p.c_vcf), (p.t_vcf, p.c_bcf), (p.t_bcf, p.c_bcf)):
            got = _same(tmp_path, t, c, want=want, batch_records=16, **m)
            assert got[4][:3] == (60 * (t == p.t_bcf), 60 * (c == p.c_bcf), nonplain)
            assert (got[4][4] > 0) == (t == p.t_vcf or c == p.c_vcf) and got[4][3] > 0


def test_bgzf_inflated_on_the_device(odd_pair, tmp_path):
    p = odd_pair
    want = _device(p.t_bcf, p.c_bcf, str(tmp_path / "want.tsv"), bcf_direct=False, do_gq=2, per_site=True)
    for inflate in (False, True):
        got = _same(tmp_path, p.t_bgzf, p.c_bgzf, want=want, device_inflate=inflate, do_gq=2, per_site=True)
        assert got[0] == 0 and got[4][:3] == (60, 60, p.not_plain(2)[0])


# ---- fallback and stop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["missing_beside_three_digits", "pl_of_five_digits", "allele_sixteen"])
def test_one_record_for_the_host_at_each_place_of_a_batch(kind, tmp_path):
    mode = 8 if kind == "pl_of_five_digits" else 6
    al17 = ["A", "C", "G", "T"] + ["<N%d>" % k for k in range(12)] + ["AT"]
    for at in (0, 3, 6):
        def fields(rnd, i, tg, nal):
            gt = [[gc.gt_value(a), gc.gt_value(b, 1)] for a, b in tg]
            gq = [[rnd.randint(1, 127)] for _ in tg]
            pl = [[0, 20, 200] + [300] * (nal * (nal + 1) // 2 - 3) for _ in tg]
            t = 1
            if i == at and kind == "missing_beside_three_digits":
                gt[1], t = [gc.gt_value(-1), gc.gt_value(117)], 2
            if i == at and kind == "pl_of_five_digits":
                gt[1], pl[1][2] = [gc.gt_value(-1), gc.gt_value(0)], 10000
            if i == at and kind == "allele_sixteen":
                gt[1] = [gc.gt_value(16), gc.gt_value(0)]
            return [("GT", t, 2, gt)] + ([("PL", 2, len(pl[0]), pl)] if mode == 8 else [("GQ", 1, 1, gq)])
        name = "f%d" % at
        samples, trecs, crecs = gc.simple_pair(tmp_path, name, 5, 7, 20 + at, fields, nal=3, alleles=(lambda i: al17) if kind == "allele_sixteen" else None)
        p = gc.Pair(tmp_path, name, samples, trecs, crecs, has_gq=mode != 8, has_pl=mode == 8)
        assert p.not_plain(mode) == (1, 7)
        got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=7, do_gq=mode, per_site=True)
        assert got[0] == 0 and got[4][:3] == (7, 7, 1), got[3][-1500:]


def test_a_stop_inside_a_batch(tmp_path):
    def fields(rnd, i, tg, nal):
        return [("GT", 1, 2, [[gc.gt_value(a), gc.gt_value(b)] for a, b in tg]), ("GQ", 1, 1, [[rnd.randint(1, 127)] for _ in tg])]
    samples, trecs, crecs = gc.simple_pair(tmp_path, "st", 5, 9, 31, fields)
    trecs[5].fields[0][3][2][1] = gc.gt_value(-1)                      # a truth genotype with a missing allele, record 6 of 9: batch 2 of 3
    p = gc.Pair(tmp_path, "st", samples, trecs, crecs, has_pl=False)
    got = _same(tmp_path, p.t_bcf, p.c_bcf, batch_records=4, do_gq=2, per_site=True)
    res = gm.compare(p.t_vcf, p.c_vcf, 2, per_site=True)
    assert got[0] == 1 and "the true genotype is missing" in got[3] and res.stop.pos == 6
    assert got[1].decode() == "".join(res.listing) and got[2] == "".join(res.per_site) and len(got[2]) > 0


# ---- the simulator's own truth file ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(VCFGL), reason="vcfgl_hip not built")
def test_tie_to_the_simulator(tmp_path):
    """vcfgl_hip -O b -printTruth 1 writes truth.bcf; a call file made of its genotypes, written as BCF, gives under --bcf-direct 1
    the tables the text forms give"""
    if _gave_up:
        pytest.fail("an earlier GPU process faulted: not started")
    for o in ("v", "b"):
        r = subprocess.run([VCFGL, "-i", DATA3, "-o", str(tmp_path / o), "-O", o, "--seed", "1", "-e", "0.01", "-d", "inf", "-printTruth", "1", "-explode", "1"],
                           capture_output=True, text=True, timeout=TIMEOUT)
        _check_alive(r.returncode, "vcfgl_hip")
        assert r.returncode == 0, r.stderr[-1000:]
    truth_v, truth_b = str(tmp_path / "v.truth.vcf"), str(tmp_path / "b.truth.bcf")
    lines = []
    for ln in open(truth_v).read().split("\n"):
        if ln.startswith("#CHROM"):
            lines.append('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">')
        if ln and not ln.startswith("#"):
            f = ln.split("\t")
            f[8] = "GT:GQ"
            f[9:] = [x.split(":")[0] + ":%d" % (1 + (7 * i + len(lines)) % 127) for i, x in enumerate(f[9:])]
            if len(lines) % 3 == 0:
                f[9] = "./.:."
            ln = "\t".join(f)
        lines.append(ln)
    call_v, call_b = str(tmp_path / "call.vcf"), str(tmp_path / "call.bcf")
    open(call_v, "w").write("\n".join(lines))
    samples, recs = gc.from_text(call_v)
    open(call_b, "wb").write(gc.bcf_bytes(samples, recs, True, False))
    for m in (dict(do_gq=0), dict(do_gq=6), dict(do_gq=2, per_site=True)):
        want = _device(truth_v, call_v, str(tmp_path / "want.tsv"), bcf_direct=False, **m)
        got = _same(tmp_path, truth_b, call_b, want=want, **m)
        assert got[0] == 0 and got[4][2] == 0 and got[4][0] == got[4][1] > 0 and got[4][4] == 0 and len(got[1]) > 0
