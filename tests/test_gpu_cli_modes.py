"""vcfgl_hip with several device stages at once writes what the run with every --device-* flag at 0 writes: the combinations that share
one allocation, one worker loop and one writer (--device-text / --device-bcf with --device-stream, --device-bgzf, --device-pileup,
--device-input and --gt-discordance; --device-gvcf with --device-bcf and --device-pileup; --records 0; the host read dumps beside a
device record path).  Every other test pins one stage at a time against the host path.

Shape: data3.vcf (4 records, 2 samples, contig length 10) with -explode 1 is 10 sites; --tile-sites 1 --devices 0,0 makes them 10 tiles
over a ring of at most 6 entries (3 per context under --device-stream 1), so every ring entry is reused, both workers run, the stream's
retire-one-behind path wraps and every gVCF block is carried across tiles and across the two workers.

Ten sites give at most ten records: "more than 10" is counted as the tests this one borrows run() / body() from count it (the lines
of body(), header included; more than 100 bytes of BCF records), and the number of records itself is pinned beside it (one per site;
for gVCF at least one block and fewer records than sites).  No combination below is refused by the argument parser: none was dropped."""
import gzip
import os

import pytest

import bcf_reader
import test_gpu_cli_bcf as tcb
import test_gpu_cli_vcftext as tcv

pytestmark = pytest.mark.gpu
INPUT = ["-i", os.path.join(tcv.DATA, "data3.vcf"), "-explode", "1", "--error-rate", "0.01"]
SHAPE = ["--tile-sites", "1", "--devices", "0,0"]          # (after run()'s own --tile-sites 7: the last value of a flag holds)
EXT = {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}
SITES = 10
DEVICE_FLAGS = ("--device-bgzf", "--device-text", "--device-bcf", "--device-gvcf", "--device-pileup", "--device-stream", "--device-input",
                "--device-inflate")
HOST = [x for f in DEVICE_FLAGS for x in (f, "0")]


def outputs(prefix, mode, r):
    """everything a run wrote, as the tests of the single stages compare it"""
    ext = EXT[mode]
    rec = tcb.stream(prefix + ext) if ext == ".bcf" else tcv.body(prefix + ext)
    truth = None
    if os.path.exists(prefix + ".truth" + ext):
        truth = tcb.stream(prefix + ".truth" + ext) if ext == ".bcf" else tcv.body(prefix + ".truth" + ext)
    pileup = gzip.open(prefix + ".pileup.gz").read() if os.path.exists(prefix + ".pileup.gz") else None
    disc = open(prefix + ".discordance.tsv").read() if os.path.exists(prefix + ".discordance.tsv") else None
    return {"records": rec, "stdout": r.stdout, "pileup": pileup, "truth": truth, "discordance": disc}


def n_records(prefix, mode):
    if EXT[mode] == ".bcf":
        return len(list(bcf_reader.Reader(prefix + ".bcf").records()))
    return len([l for l in tcv.body(prefix + EXT[mode]) if not l.startswith("#")])


def host_and_device(tmp_path, mode, flags, device):
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = tcv.run(a, mode, INPUT + flags, SHAPE + HOST)
    rb = tcv.run(b, mode, INPUT + flags, SHAPE + device)
    oa, ob = outputs(a, mode, ra), outputs(b, mode, rb)
    for k in oa:
        assert oa[k] == ob[k], k
    if EXT[mode] == ".bcf":
        assert len(oa["records"][1]) > 100
    else:
        assert len(oa["records"]) > 10
    return a, oa


TAGS = ["--depth", "4", "--gt-discordance", "1", "-printPileup", "1", "-printTruth", "1", "-addPL", "1", "-addQS", "1", "-addInfoAD", "1"]
STAGES = ["--device-stream", "1", "--device-bgzf", "1", "--device-pileup", "1", "--device-input", "1"]


@pytest.mark.parametrize("mode,record_flag", [("z", "--device-text"), ("b", "--device-bcf")])
def test_every_stage_of_a_compressed_run_at_once(mode, record_flag, tmp_path):
    a, o = host_and_device(tmp_path, mode, TAGS, [record_flag, "1"] + STAGES)
    assert n_records(a, mode) == SITES
    assert o["pileup"].count(b"\n") == SITES and o["truth"] is not None and o["discordance"]


def test_device_gvcf_bcf_and_pileup_with_every_block_carried(tmp_path):
    flags = ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1", "-doUnobserved", "2", "--depth", "2", "-printPileup", "1"]
    a, o = host_and_device(tmp_path, "u", flags, ["--device-gvcf", "1", "--device-bcf", "1", "--device-pileup", "1"])
    recs = list(bcf_reader.Reader(a + ".bcf").records())
    assert 1 < len(recs) < SITES                                   # blocks were merged, and not into one
    assert any(k == "MIN_DP" for r in recs for k, _, _ in r["info"])
    assert o["pileup"].count(b"\n") == SITES


def test_records_0_over_two_contexts_tallies_what_a_run_with_records_tallies(tmp_path):
    a, b = str(tmp_path / "one"), str(tmp_path / "two")
    flags = INPUT + ["--depth", "4", "--gt-discordance", "1", "--tile-sites", "1"]
    tcv.run(a, "b", flags, ["--records", "1"])
    tcv.run(b, "b", flags, ["--records", "0", "--devices", "0,0"])
    want = open(a + ".discordance.tsv").read()
    assert want.count("\n") == 2 and open(b + ".discordance.tsv").read() == want
    assert os.path.exists(a + ".bcf") and n_records(a, "b") == SITES
    assert not [f for f in os.listdir(tmp_path) if f.startswith("two") and not f.endswith((".arg", ".discordance.tsv"))]


def test_host_read_dumps_beside_device_text(tmp_path):
    flags = ["--depth", "4", "--error-qs", "2", "--beta-variance", "1e-4", "-printPileup", "1", "--adjust-qs", "4", "-printQScores", "1",
             "-printQsError", "1"]
    a, o = host_and_device(tmp_path, "v", flags, ["--device-text", "1", "--device-pileup", "0"])
    assert n_records(a, "v") == SITES
    assert o["stdout"].count("\n") > 10 and o["pileup"].count(b"\n") == SITES
