"""vcfgl_hip --device-bcf-input 1 (the genotypes of a BCF input decoded on the device) writes what --device-bcf-input 0 writes: over the
reference's golden configurations in its own draw order with the BCF made from each input, raw and BGZF; on a synthetic BCF through
the device record path and through the discordance table, also behind --device-inflate 1; on a hand-built file of odd records whose
fallback records are counted; on a truncated file; through --dump-gt; and the flag's refusals."""
import os
import re

import pytest

import bcfin_cases as bc
import bcfin_model as bm
import golden_util as gu
import inflate_corpus as ic
import synth
import test_bcfin_cpu as tbc
import test_gpu_cli_input as tci

pytestmark = pytest.mark.gpu
DATA = tci.DATA
run, same_outputs = tci.run, tci.same_outputs


def input_line(stderr):
    """(records decoded on the device, records decoded again on the host) of the flag's [input] line"""
    m = re.search(r"^\[input\] --device-bcf-input 1: (\d+) records decoded on the device, (\d+) of them again on the host, ([0-9.]+) GB of genotype "
                  r"bytes sent up; no fallback; header and record chain [0-9.]+ s, shared blocks [0-9.]+ s, device decode and wait [0-9.]+ s, "
                  r"host GT loop [0-9.]+ s$", stderr, re.M)
    assert m, stderr[-1500:]
    return int(m.group(1)), int(m.group(2))


@pytest.fixture(scope="module")
def golden_bcfs(tmp_path_factory):
    """the BCF of every golden input, raw and BGZF (read with --source 1: a --source 0 input comes back with the alleles A, C)"""
    d = tmp_path_factory.mktemp("golden_bcf")
    inputs = sorted({gu.REF_TESTS[n]["input"] for n in tci.GOLD})
    return {(name, mode): tbc.golden_bcf(os.path.join(DATA, name), mode, d) for name in inputs for mode in ("u", "b")}


@pytest.mark.parametrize("mode", ["u", "b"])
@pytest.mark.parametrize("name", tci.GOLD)
def test_golden_configurations(name, mode, golden_bcfs, tmp_path):
    t = gu.REF_TESTS[name]
    argv, toks = [], t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        if flag == "--source":
            continue
        argv += [flag, val]
    bcf = golden_bcfs[(t["input"], mode)]
    res = {}
    for k in ("0", "1"):
        res[k] = run(["-i", bcf, "-o", str(tmp_path / ("o" + k)), "--rng-mode", "1", "--verbose", "1", "--source", "1", "--device-bcf-input", k] + argv)
    exts = same_outputs("o0", "o1", tmp_path)
    assert ".vcf" in exts and ("-printTruth" not in toks or ".truth.vcf" in exts) and ("-printPileup" not in toks or ".pileup.gz" in exts)
    assert res["0"].stdout == res["1"].stdout
    n_dev, n_host = input_line(res["1"].stderr)
    assert n_host == 0 and n_dev == len(bm.parse_bcf(bm.read_raw(bcf))[1]) > 0
    assert "--device-bcf-input" not in res["0"].stderr.split("[timing]")[-1]      # the line is printed only with the flag


@pytest.fixture(scope="module")
def synth_bcf(tmp_path_factory):
    """700 sites x 257 samples of phased binary genotypes as int8 pairs, raw and BGZF"""
    S, N = 700, 257
    gt = synth.binary_sites(0, S, N)
    d = tmp_path_factory.mktemp("synth")
    data = bc.binary_bcf(gt)
    raw, bgzf = str(d / "in.bcf"), str(d / "in.bgzf.bcf")
    open(raw, "wb").write(data)
    open(bgzf, "wb").write(ic.bgzf_level6(data))
    return raw, bgzf, S, N, gt


FLAGS = "--seed 42 --depth 4 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -addPL 1 --tile-sites 256 --source 1 --verbose 1".split()
RECORD_PATH = ["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]
TABLE_ONLY = ["--records", "0", "--gt-discordance", "1"]


@pytest.mark.parametrize("inflate", ["0", "1"])
@pytest.mark.parametrize("path_flags,exts", [(RECORD_PATH, [".bcf"]), (TABLE_ONLY, [".discordance.tsv"])], ids=["records", "table"])
def test_synthetic_bcf(path_flags, exts, inflate, synth_bcf, tmp_path):
    raw, bgzf, S, N, gt = synth_bcf
    src = bgzf if inflate == "1" else raw
    res = {k: run(["-i", src, "-o", str(tmp_path / ("o" + k)), "--device-inflate", inflate, "--device-bcf-input", k] + path_flags + FLAGS) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == exts and os.path.getsize(str(tmp_path / ("o1" + exts[0]))) > 10000
    assert input_line(res["1"].stderr) == (S, 0)                          # three batches of at most 256 records
    if inflate == "1":
        assert "no fallback; inflate stage" in res["1"].stderr


def test_dump_gt_of_the_synthetic_bcf(synth_bcf):
    raw, bgzf, S, N, gt = synth_bcf
    dev = tbc.dump(raw, 1, 2)
    assert dev == tbc.dump(raw, 1, 3) == tbc.dump(bgzf, 1, 2)
    assert [l.split(" ", 2)[2] for l in dev.splitlines()] == [l.split(" ", 2)[2] for l in tbc.dump(raw, 1, 0).splitlines()]
    rows = dev.split("\n")
    assert len(rows) == S + 1 and rows[5].split() == ["6", "0", str(int((gt[5] & 1).sum() + (gt[5] >> 4).sum())), bytes(gt[5]).hex()]


def test_odd_records_and_the_fallback_count(tmp_path):
    path, fallback = tbc.write_odd_bcf(tmp_path)
    flags = "--seed 7 --depth 3 -e 0.01 --source 1 -O v -printTruth 1 -addPL 1 --tile-sites 4 --verbose 1".split()
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--device-bcf-input", k] + flags) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".truth.vcf", ".vcf"]
    assert input_line(res["1"].stderr) == (len(bc.ODD_RECORDS), len(fallback)) and len(fallback) == 3
    truth = [l.split("\t")[9:] for l in open(str(tmp_path / "o1.truth.vcf")).read().splitlines() if l.startswith("chr22\t8\t")]
    assert truth == [["0|1/1", "1|1", "2|2/.", "0", "3|4/9"]]             # the GT text is the host's, values behind the second included
    want = bm.dump_text(bm.file_rows(open(path, "rb").read(), 1))
    assert tbc.dump(path, 1, 2) == want == tbc.dump(path, 1, 3)


@pytest.mark.parametrize("name", sorted({gu.REF_TESTS[n]["input"] for n in tci.GOLD}))
def test_dump_gt_on_the_golden_inputs(name, golden_bcfs):
    for mode in ("u", "b"):
        bcf = golden_bcfs[(name, mode)]
        dev = tbc.dump(bcf, 1, 2)
        assert dev == tbc.dump(bcf, 1, 3)                                 # rows, sums and statuses
        # ... 0 is today's reader: the same positions, sums and rows (it gives a BCF record no status)
        assert [l.split(" ", 2)[2] for l in dev.splitlines()] == [l.split(" ", 2)[2] for l in tbc.dump(bcf, 1, 0).splitlines()]
        assert [l.split(" ")[0] for l in dev.splitlines()] == [l.split(" ")[0] for l in tbc.dump(bcf, 1, 0).splitlines()]


@pytest.mark.parametrize("cut", ["in the last record", "in a record's lengths", "in the header"])
def test_a_truncated_bcf_gives_the_message_and_the_files_of_the_host_reader(cut, synth_bcf, tmp_path):
    raw = open(synth_bcf[0], "rb").read()
    rec = (len(raw) - 9 - int.from_bytes(raw[5:9], "little")) // synth_bcf[2]          # every record has the same size
    n = {"in the last record": len(raw) - 100, "in a record's lengths": len(raw) - rec + 5, "in the header": 200}[cut]
    path = str(tmp_path / "cut.bcf")
    open(path, "wb").write(raw[:n])
    msgs = []
    for k in ("0", "1"):
        r = run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--device-bcf-input", k] + TABLE_ONLY + FLAGS, ok=False)
        assert r.returncode != 0
        msgs.append(r.stderr[r.stderr.index("[ERROR]"):])
    assert msgs[0] == msgs[1] and "truncated BCF" in msgs[0]
    assert not [f for f in os.listdir(str(tmp_path)) if not f.endswith((".arg", "cut.bcf"))]


def test_a_record_the_host_reader_exits_on_sends_the_whole_file_to_it(tmp_path):
    """an allele index beyond the record's alleles: handed back by the device, make_site's exit as with the flag off"""
    data, _ = bc.odd_bcf()
    data += bc.bcf_record(16, bc.ODD_ALLELES[:2], 5, [(bc.GT, 1, 2, bytes([2, 4, 2, 2, 2, 2, 2, 7, 2, 2]))])      # 0/2 of G,T
    path = str(tmp_path / "bad.bcf")
    open(path, "wb").write(data)
    msgs = []
    for k in ("0", "1"):
        r = run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--seed", "7", "--depth", "3", "-e", "0.01", "--source", "1", "-O", "v", "--device-bcf-input", k], ok=False)
        assert r.returncode != 0
        msgs.append(r.stderr[r.stderr.index("[ERROR]"):])
    assert msgs[0] == msgs[1] and "GT allele index out of range at position 16" in msgs[0]


def test_text_input_and_depth_inf_are_refused(golden_bcfs, tmp_path):
    bcf = golden_bcfs[("data2.vcf", "u")]
    base = ["--seed", "1", "-e", "0.01", "--source", "1", "-O", "v", "--device-bcf-input", "1"]
    r = run(["-i", os.path.join(DATA, "data2.vcf"), "-o", str(tmp_path / "t"), "--depth", "1"] + base, ok=False)
    assert r.returncode != 0 and "--device-bcf-input 1 needs BCF input" in r.stderr
    r = run(["-i", bcf, "-o", str(tmp_path / "i"), "--depth", "inf"] + base, ok=False)
    assert r.returncode != 0 and "--device-bcf-input 1 is not supported with --depth inf" in r.stderr
    assert os.listdir(str(tmp_path)) == []                               # nothing was created, not even an .arg file
    run(["-i", bcf, "-o", str(tmp_path / "ok"), "--depth", "1"] + base)
    assert os.path.getsize(str(tmp_path / "ok.vcf")) > 1000
