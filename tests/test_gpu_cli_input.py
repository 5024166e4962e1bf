"""vcfgl_hip --device-input 1 (the genotype columns of the input VCF parsed on the device) writes what --device-input 0 writes: over
the reference's golden configurations in its own draw order, on a synthetic input through the device record path and through the
discordance table, on a file of odd lines whose fallback lines are counted, through --dump-gt, and BCF input is refused."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import synth
import test_vcfin_cpu as tvc
import vcfin_cases as vc

pytestmark = pytest.mark.gpu
BIN = tvc.BIN
DATA = os.path.join(gu.REFVCF, "data")


def run(argv, ok=True):
    r = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def input_line(stderr):
    """(lines parsed on the device, lines parsed again on the host) of the [input] line"""
    m = re.search(r"^\[input\] --device-input 1: (\d+) lines parsed on the device, (\d+) of them again on the host, ([0-9.]+) GB of text sent up; "
                  r"file read [0-9.]+ s, line scan [0-9.]+ s, fixed columns [0-9.]+ s, device parse and wait [0-9.]+ s, host re-parse [0-9.]+ s$",
                  stderr, re.M)
    assert m, stderr[-1500:]
    return int(m.group(1)), int(m.group(2))


def payload(path):
    """what a produced file holds, apart from its ## header lines"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    if raw[:3] == b"BCF":
        l_text = int.from_bytes(raw[5:9], "little")
        hdr = b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##"))
        return hdr + raw[9 + l_text:]
    return b"\n".join(l for l in raw.split(b"\n") if not l.startswith(b"##"))


def same_outputs(a, b, tmp_path):
    """every file of prefix a has a twin of prefix b with the same payload (the .arg files record the command lines)"""
    fa = sorted(f[len(a):] for f in os.listdir(str(tmp_path)) if f.startswith(a) and not f.endswith(".arg"))
    fb = sorted(f[len(b):] for f in os.listdir(str(tmp_path)) if f.startswith(b) and not f.endswith(".arg"))
    assert fa == fb and fa
    for ext in fa:
        assert payload(str(tmp_path / (a + ext))) == payload(str(tmp_path / (b + ext))), ext
    return fa


# the configurations that write VCF text or gVCF (none of the recorded ones writes BCF; --depth inf, which the flag refuses, is not among them)
GOLD = [n for n in sorted(gu.REF_TESTS, key=lambda s: int(s[4:])) if "inf" not in gu.REF_TESTS[n]["args"].split()]
assert len(GOLD) == len(gu.REF_TESTS) == 17, "a recorded configuration dropped out of (or joined) the --device-input comparison: look at it"


@pytest.mark.parametrize("name", GOLD)
def test_golden_configurations(name, tmp_path):
    t = gu.REF_TESTS[name]
    argv, toks = [], t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        argv += [flag, val]
    assert len(GOLD) >= 15 and {"test2", "test3", "test7", "test10", "test14", "test18"} <= set(GOLD)    # -printTruth, --rm-invar-sites 3, gVCF, pileup, --source 0, -explode
    res = {}
    for k in ("0", "1"):
        res[k] = run(["-i", os.path.join(DATA, t["input"]), "-o", str(tmp_path / ("o" + k)), "--rng-mode", "1", "--verbose", "1", "--device-input", k] + argv)
    exts = same_outputs("o0", "o1", tmp_path)
    assert ".vcf" in exts and ("-printTruth" not in toks or ".truth.vcf" in exts) and ("-printPileup" not in toks or ".pileup.gz" in exts)
    assert res["0"].stdout == res["1"].stdout
    n_dev, n_host = input_line(res["1"].stderr)
    assert n_host == 0 and n_dev == len(tvc.vm.read_lines(os.path.join(DATA, t["input"]))[2]) > 0
    assert "[input] --device-input 0: 0 lines parsed on the device" in res["0"].stderr


@pytest.fixture(scope="module")
def synth_vcf(tmp_path_factory):
    """700 sites x 257 samples of phased binary genotypes, gzip-compressed"""
    S, N = 700, 257
    gt = synth.binary_sites(0, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    path = str(tmp_path_factory.mktemp("synth") / "in.vcf.gz")
    with gzip.open(path, "wt", compresslevel=1) as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        for i in range(S):
            idx = (gt[i] & 0xF).astype(np.int64) + 2 * (gt[i] >> 4).astype(np.int64)
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
    return path, S, N, gt


FLAGS = "--seed 42 --depth 4 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -addPL 1 --tile-sites 256 --verbose 1".split()


def test_synthetic_input_through_the_device_record_path(synth_vcf, tmp_path):
    path, S, N, gt = synth_vcf
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1",
                   "--device-input", k] + FLAGS) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".bcf"] and os.path.getsize(str(tmp_path / "o1.bcf")) > 10000
    assert input_line(res["1"].stderr) == (S, 0)                          # three batches of at most 256 lines


def test_synthetic_input_through_the_discordance_table(synth_vcf, tmp_path):
    path, S, N, gt = synth_vcf
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--records", "0", "--gt-discordance", "1", "--device-input", k] + FLAGS) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".discordance.tsv"]
    assert len(open(str(tmp_path / "o1.discordance.tsv")).read().split("\n")) > N
    assert input_line(res["1"].stderr) == (S, 0)


def test_dump_gt_of_the_synthetic_input(synth_vcf):
    path, S, N, gt = synth_vcf
    dev = tvc.dump(path, 0, 1)
    assert dev == tvc.dump(path, 0, 0)
    rows = dev.split("\n")
    assert len(rows) == S + 1 and rows[5].split() == ["6", "0", str(int((gt[5] & 1).sum() + (gt[5] >> 4).sum())), bytes(gt[5]).hex()]


def test_odd_lines_and_the_fallback_count(tmp_path):
    path, fallback = tvc.write_odd_lines(tmp_path)
    flags = "--seed 7 --depth 3 -e 0.01 --source 1 -O v -printTruth 1 -addPL 1 --tile-sites 4 --verbose 1".split()
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--device-input", k] + flags) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".truth.vcf", ".vcf"]
    assert input_line(res["1"].stderr) == (len(vc.ODD_LINES), len(fallback))
    want = tvc.vm.dump_text(tvc.vm.file_rows(path, 1))
    assert tvc.dump(path, 1, 1) == want == tvc.dump(path, 1, 0)


@pytest.mark.parametrize("path", tvc.GOLDEN, ids=tvc.IDS)
def test_dump_gt_on_the_golden_inputs(path):
    source = tvc._source(path)
    assert tvc.dump(path, source, 1) == tvc.dump(path, source, 0)


def test_a_line_with_another_column_count_exits_as_with_the_host_parser(tmp_path):
    path = os.path.join(DATA, "data8.vcf")
    msgs = []
    for k in ("0", "1"):
        r = run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--seed", "1", "--depth", "1", "-e", "0.01", "--source", "1", "-O", "v", "--device-input", k], ok=False)
        assert r.returncode != 0
        msgs.append(re.sub(r"position \d+", "position P", r.stderr[r.stderr.index("[ERROR]"):]))      # (whichever thread meets its line first)
    assert msgs[0] == msgs[1] and "has 10 sample columns, the header names 9 samples" in msgs[0]
    assert not [f for f in os.listdir(str(tmp_path)) if not f.endswith(".arg")]


def test_bcf_input_is_refused(tmp_path):
    src = str(tmp_path / "in")
    run(["-i", os.path.join(DATA, "data2.vcf"), "-o", src, "--seed", "1", "--depth", "inf", "-e", "0", "-O", "u", "-printTruth", "1"])
    bcf = src + ".truth.bcf"                                             # (the truth file keeps GT: a BCF the program reads)
    assert open(bcf, "rb").read(3) == b"BCF"
    run(["-i", bcf, "-o", str(tmp_path / "ok"), "--seed", "1", "--depth", "1", "-e", "0.01", "--source", "1", "-O", "v"])
    before = set(os.listdir(str(tmp_path)))
    r = run(["-i", bcf, "-o", str(tmp_path / "refused"), "--seed", "1", "--depth", "1", "-e", "0.01", "--source", "1", "-O", "v", "--device-input", "1"], ok=False)
    assert r.returncode != 0 and "--device-input 1 is not supported with BCF input" in r.stderr
    assert set(os.listdir(str(tmp_path))) == before                      # not even the .arg file
