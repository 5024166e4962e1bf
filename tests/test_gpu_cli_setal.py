"""vcfgl_hip --set-alleles FILE: the record file of a run with the flag equals the model of misc/setAlleles (tests/setal_model.py)
applied to the record file of the same run without it, value for value; the text outputs are the writers' formatting of those same
values; every path that writes records gives the same bytes; the side files are unchanged; and everything the flag does not support
is refused with its reason."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bcf_reader
import golden_util as gu
import setal_model as sm
import vcftext_model as vt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
INPUT = os.path.join(gu.REFVCF, "data", "data3.vcf")
NAMES = ["A", "C", "G", "T", "<*>"]
BASE = ["--seed", "42", "-e", "0.05", "-d", "3", "-explode", "1", "--tile-sites", "3", "-doUnobserved", "4", "-addPL", "1", "-addGP", "1", "-addQS", "1",
        "-addInfoDP", "1"]


def run(out, *flags, ok=True):
    r = subprocess.run([BIN, "-i", INPUT, "-o", out] + list(flags), capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def records(path):
    return list(bcf_reader.Reader(path).records())


def text_lines(path):
    data = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
    return [ln for ln in data.decode().split("\n") if ln and not ln.startswith("##source=")]


def bcf_body(path):
    r = bcf_reader.Reader(path)
    return [h for h in r.header if not h.startswith("##source=")], r.raw[r.off:]


def write_tsv(path, recs, seed):
    """for every record a random arrangement of some of its own alleles: 2, 3, 4, 5, 2, ... of them (as many as it has, at most)"""
    rng = np.random.default_rng(seed)
    targets = []
    with open(path, "w") as f:
        for i, r in enumerate(recs):
            t = [str(x) for x in rng.permutation(r["alleles"])[:min(2 + i % 4, len(r["alleles"]))]]
            targets.append(t)
            f.write(t[0] + "\t" + ",".join(t[1:]) + "\n")
    return targets


def per_tag(rec, key):
    return next(p for k, t, p in rec["fmt"] if k == key)


def model_record(rec, target):
    old, new = [NAMES.index(a) for a in rec["alleles"]], [NAMES.index(a) for a in target]
    bits = lambda key: np.array(per_tag(rec, key), np.uint32).T.copy()
    pl = np.array([[-2 ** 31 if x is None else x for x in v] for v in per_tag(rec, "PL")], np.int32).T.copy()
    qs = np.array(next(v for k, t, v in rec["info"] if k == "QS"), np.uint32).view(np.float32)
    return sm.relabel_record(old, new, qs=qs, gl=bits("GL"), pl=pl.view(np.uint32), gp=bits("GP"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """per RNG mode: the plain -O u run, the allele file made from its records, and the flagged -O u run: made once, shared"""
    d = tmp_path_factory.mktemp("setal_cli")
    out = {}
    for mode in ("0", "1"):
        o = lambda k: str(d / (k + mode))
        run(o("plain"), "-O", "u", "--rng-mode", mode, *BASE)
        plain = records(o("plain") + ".bcf")
        tsv = o("alleles") + ".tsv"
        targets = write_tsv(tsv, plain, 7 + int(mode))
        run(o("flag"), "-O", "u", "--rng-mode", mode, "--set-alleles", tsv, *BASE)
        out[mode] = dict(dir=d, plain=plain, tsv=tsv, targets=targets, flag=o("flag") + ".bcf")
    return out


@pytest.mark.parametrize("mode", ["0", "1"])
def test_flagged_bcf_equals_the_model_of_the_plain_bcf(runs, mode):
    R = runs[mode]
    got = records(R["flag"])
    assert len(got) == len(R["plain"]) == len(R["targets"]) == 10
    assert {len(t) for t in R["targets"]} == {2, 3, 4, 5}
    for rec, tgt, g in zip(R["plain"], R["targets"], got):
        want = model_record(rec, tgt)
        assert g["alleles"] == tgt and (g["chrom"], g["pos0"], g["id"], g["filter"]) == (rec["chrom"], rec["pos0"], rec["id"], rec["filter"])
        assert per_tag(g, "DP") == per_tag(rec, "DP")
        assert [v for k, t, v in g["info"] if k == "DP"] == [v for k, t, v in rec["info"] if k == "DP"]
        assert next(v for k, t, v in g["info"] if k == "QS") == [int(b) for b in want["qs"].view(np.uint32)]
        for key, kind in (("GL", "gl"), ("GP", "gp")):
            assert per_tag(g, key) == [[int(b) for b in want[kind][:, s]] for s in range(want[kind].shape[1])], key
        wpl = want["pl"].view(np.int32)
        assert per_tag(g, "PL") == [[None if v == -2 ** 31 else int(v) for v in wpl[:, s]] for s in range(wpl.shape[1])]


def test_text_outputs_are_the_writers_formatting_of_the_relabelled_values(runs):
    R = runs["0"]
    o = lambda k: str(R["dir"] / k)
    want = list(bcf_reader.Reader(R["flag"]).vcf_lines(vt.fmt_float_bits))
    for mode, ext in (("v", ".vcf"), ("z", ".vcf.gz")):
        run(o("t" + mode), "-O", mode, "--rng-mode", "0", "--set-alleles", R["tsv"], *BASE)
        got = [ln for ln in text_lines(o("t" + mode) + ext) if not ln.startswith("#")]
        assert got == want, mode
    run(o("tb"), "-O", "b", "--rng-mode", "0", "--set-alleles", R["tsv"], *BASE)
    assert records(o("tb") + ".bcf") == records(R["flag"])


def test_every_path_writes_the_same_bytes(runs):
    R = runs["0"]
    o = lambda k: str(R["dir"] / k)
    flags = ["--rng-mode", "0", "--set-alleles", R["tsv"]] + BASE
    run(o("hv"), "-O", "v", *flags)
    host_v = text_lines(o("hv") + ".vcf")
    host_u = bcf_body(R["flag"])
    cases = [("v", ["--device-text", "1"]), ("z", ["--device-text", "1"]), ("z", ["--device-text", "1", "--device-stream", "1"]),
             ("z", ["--device-text", "1", "--device-stream", "1", "--device-bgzf", "1"]), ("v", ["--devices", "0,0"]),
             ("u", ["--device-bcf", "1"]), ("b", ["--device-bcf", "1"]), ("b", ["--device-bcf", "1", "--device-stream", "1"]),
             ("b", ["--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]), ("u", ["--devices", "0,0"]),
             ("b", ["--device-bcf", "1", "--device-stream", "1", "--devices", "0,0"])]
    for k, (mode, extra) in enumerate(cases):
        run(o("p%d" % k), "-O", mode, *extra, *flags)
        if mode in "vz":
            assert text_lines(o("p%d" % k) + (".vcf" if mode == "v" else ".vcf.gz")) == host_v, (mode, extra)
        else:
            assert bcf_body(o("p%d" % k) + ".bcf") == host_u, (mode, extra)


def test_truth_and_pileup_files_are_unchanged(runs):
    R = runs["0"]
    o = lambda k: str(R["dir"] / k)
    side = ["-O", "v", "--rng-mode", "0", "-printTruth", "1", "-printPileup", "1"] + BASE
    run(o("s0"), *side)
    run(o("s1"), "--set-alleles", R["tsv"], *side)
    assert text_lines(o("s0") + ".truth.vcf") == text_lines(o("s1") + ".truth.vcf")
    assert gzip.open(o("s0") + ".pileup.gz").read() == gzip.open(o("s1") + ".pileup.gz").read()


def test_everything_unsupported_is_refused_with_its_reason(runs, tmp_path):
    R = runs["0"]
    tsv = R["tsv"]
    base = ["-O", "v", "--set-alleles", tsv]
    swap = lambda flags, key, val: [val if i and flags[i - 1] == key else x for i, x in enumerate(flags)]
    cases = [(swap(BASE, "-d", "inf"), "--depth inf"),
             (BASE + ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addFormatDP", "1"], "-doGVCF 1"),
             (BASE + ["--rm-empty-sites", "1"], "--rm-empty-sites 1"),
             (BASE + ["--rm-invar-sites", "4"], "--rm-invar-sites 4"),
             (BASE + ["-addFormatAD", "1"], "the AD / ADF / ADR"), (BASE + ["-addInfoAD", "1"], "the AD / ADF / ADR"),
             (BASE + ["-addFormatADF", "1"], "the AD / ADF / ADR"), (BASE + ["-addInfoADR", "1"], "the AD / ADF / ADR"),
             (BASE + ["--gt-discordance", "1"], "--gt-discordance 1"),
             (BASE + ["--fetch-gl", "AC"], "--fetch-gl AC"),
             (BASE + ["--fetch-gl", "AC", "--records", "0"], "--fetch-gl AC"),
             (BASE + ["--records", "0"], "--records 0")]
    for k, (flags, msg) in enumerate(cases):
        r = run(str(tmp_path / ("r%d" % k)), *base, *flags, ok=False)
        assert "--set-alleles" in r.stderr and "not supported with " + msg in r.stderr, (flags, r.stderr[-600:])
        assert not os.path.exists(str(tmp_path / ("r%d" % k)) + ".vcf")


def test_a_bad_allele_file_stops_the_run_with_a_clear_message(runs, tmp_path):
    good = open(runs["0"]["tsv"]).read().splitlines()
    files = {"short": (good[:-1], "has 9 lines but the run has more records"),
             "long": (good + ["A\tC"], "has 11 lines but the run has 10 records"),
             "notab": (["A C"] + good[1:], "line 1: expected REF<TAB>ALT"),
             "twice": (good[:2] + ["A\tC,A"] + good[3:], "line 3: allele A is named twice"),
             "five": (["A\tC,G,T,<*>,A"] + good[1:], "line 1: 5 ALT alleles; at most 4"),
             "spelling": (["A\t<NON_REF>"] + good[1:], "the unobserved allele of this run is spelled <*>"),
             "unknown": (["A\tN"] + good[1:], "line 1: unknown allele 'N'"),
             "missing": (None, "Could not open file")}
    for name, (lines, msg) in files.items():
        p = str(tmp_path / (name + ".tsv"))
        if lines is not None:
            open(p, "w").write("\n".join(lines) + "\n")
        r = run(str(tmp_path / name), "-O", "v", "--set-alleles", p, *BASE, ok=False)
        assert msg in r.stderr, (name, r.stderr[-600:])


def test_a_target_allele_the_record_lacks_stops_the_run_naming_the_site(tmp_path):
    flags = [x for x in BASE]
    flags[flags.index("-doUnobserved") + 1] = "1"
    run(str(tmp_path / "plain"), "-O", "u", *flags)
    recs = records(str(tmp_path / "plain") + ".bcf")
    lacking = [i for i, r in enumerate(recs) if not {"A", "C", "G", "T"} <= set(r["alleles"])]
    assert lacking, "every record has A, C, G and T: the case is not exercised"
    p = str(tmp_path / "acgt.tsv")
    open(p, "w").write("A\tC,G,T\n" * len(recs))
    r = run(str(tmp_path / "bad"), "-O", "u", "--set-alleles", p, *flags, ok=False)
    assert "--set-alleles: site %d:" % lacking[0] in r.stderr and "does not have" in r.stderr, r.stderr[-600:]
