"""vcfgl_hip --device-inflate 1 (a BGZF input inflated on the device) writes what --device-inflate 0 writes: golden inputs written as
BGZF two ways, compressed BCF fed back in, inputs that are not BGZF and a damaged file (both read by zlib after all), and a file of
more members than one batch holds."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_util as gu
import inflate_corpus as ic
import synth
import test_gpu_cli_input as tci
from vcfgl_amd import bgzf

pytestmark = pytest.mark.gpu
DATA = tci.DATA
run, same_outputs = tci.run, tci.same_outputs

INFLATED = re.compile(r"^\[input\] --device-inflate 1: (\d+) members inflated on the device, (\d+) compressed bytes sent up, (\d+) inflated "
                      r"bytes received, no fallback; inflate stage [0-9.]+ s of file read [0-9.]+ s$", re.M)
FELL_BACK = re.compile(r"^\[input\] --device-inflate 1: (\d+) members inflated on the device, .* the host read the file \(zlib\): (.*); inflate stage", re.M)


def golden_argv(name):
    t = gu.REF_TESTS[name]
    argv, toks = [], t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        argv += [flag, val]
    return os.path.join(DATA, t["input"]), argv


def write_bgzf(path, data, how):
    if how == "zlib6":
        open(path, "wb").write(ic.bgzf_level6(data))
    else:
        bgzf.write_file(path, [bgzf.compress(torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda:0"))])
    assert gzip.decompress(open(path, "rb").read()) == data


@pytest.mark.parametrize("how", ["zlib6", "device"])
@pytest.mark.parametrize("name", ["test2", "test7", "test14"])          # -printTruth, gVCF, --source 0
def test_golden_inputs_as_bgzf(name, how, tmp_path):
    src, argv = golden_argv(name)
    path = str(tmp_path / "in.vcf.gz")
    write_bgzf(path, open(src, "rb").read(), how)
    res = {}
    for k, extra in (("0", []), ("1", []), ("2", ["--device-input", "1"])):
        res[k] = run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--rng-mode", "1", "--verbose", "1", "--device-inflate", "1" if k != "0" else "0"] + argv + extra)
    plain = run(["-i", src, "-o", str(tmp_path / "p"), "--rng-mode", "1"] + argv)
    exts = same_outputs("o0", "o1", tmp_path)
    assert same_outputs("o0", "o2", tmp_path) == exts == same_outputs("o0", "p", tmp_path) and ".vcf" in exts
    assert res["0"].stdout == res["1"].stdout == res["2"].stdout == plain.stdout
    for k in ("1", "2"):
        m = INFLATED.search(res[k].stderr)
        assert m and int(m.group(1)) == 2, res[k].stderr[-1500:]               # the text's member and the EOF member
    assert "[input] --device-inflate 0: the host read the file (zlib)" in res["0"].stderr
    assert tci.input_line(res["2"].stderr)[0] > 0


FLAGS = "--seed 42 --depth 4 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -addPL 1 --tile-sites 256 --verbose 1".split()


def test_more_members_than_a_batch(tmp_path):
    """700 lines x 257 samples in members of 500 bytes: two batches of 512 and one of the rest, with --device-input 1 behind them"""
    S, N = 700, 257
    gt = synth.binary_sites(0, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    text = ["##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1),
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n"]
    for i in range(S):
        idx = (gt[i] & 0xF).astype(np.int64) + 2 * (gt[i] >> 4).astype(np.int64)
        text.append("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
    data = "".join(text).encode()
    path = str(tmp_path / "in.vcf.gz")
    open(path, "wb").write(b"".join(ic.wrap(ic.deflate(data[i:i + 500]), data[i:i + 500]) for i in range(0, len(data), 500)) + ic.EOF)
    n_members = (len(data) + 499) // 500 + 1
    assert n_members > 2 * 512
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--records", "0", "--gt-discordance", "1", "--device-input", "1", "--device-inflate", k] + FLAGS)
           for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".discordance.tsv"]
    m = INFLATED.search(res["1"].stderr)
    assert m and int(m.group(1)) == n_members and int(m.group(3)) == len(data) and int(m.group(2)) == os.path.getsize(path), res["1"].stderr[-1500:]
    assert tci.input_line(res["1"].stderr) == (S, 0)


def test_compressed_bcf_fed_back_in(tmp_path):
    src = str(tmp_path / "in")
    run(["-i", os.path.join(DATA, "data2.vcf"), "-o", src, "--seed", "1", "--depth", "inf", "-e", "0", "-O", "b", "-printTruth", "1"])
    bcf = src + ".truth.bcf"                                             # (the truth file keeps GT: a BCF the program reads)
    raw = open(bcf, "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and gzip.decompress(raw)[:3] == b"BCF"
    argv = ["--seed", "1", "--depth", "2", "-e", "0.01", "--source", "1", "-O", "v", "-addPL", "1", "--verbose", "1"]
    res = {k: run(["-i", bcf, "-o", str(tmp_path / ("o" + k)), "--device-inflate", k] + argv) for k in ("0", "1")}
    assert same_outputs("o0", "o1", tmp_path) == [".vcf"] and res["0"].stdout == res["1"].stdout
    assert INFLATED.search(res["1"].stderr), res["1"].stderr[-1500:]


@pytest.mark.parametrize("kind", ["plain", "gzip"])
def test_inputs_that_are_not_bgzf_are_read_by_the_host(kind, tmp_path):
    src, argv = golden_argv("test2")
    data = open(src, "rb").read()
    path = str(tmp_path / ("in.vcf" if kind == "plain" else "in.vcf.gz"))
    open(path, "wb").write(data if kind == "plain" else gzip.compress(data))
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--rng-mode", "1", "--verbose", "1", "--device-inflate", k] + argv) for k in ("0", "1")}
    assert ".vcf" in same_outputs("o0", "o1", tmp_path) and res["0"].stdout == res["1"].stdout
    m = FELL_BACK.search(res["1"].stderr)
    assert m and int(m.group(1)) == 0 and m.group(2) == "the file is not a series of BGZF members", res["1"].stderr[-1500:]


def test_a_member_with_a_flipped_crc(tmp_path):
    """zlib stops at the bad member: both settings read the same (cut) text and end the same way"""
    lines = open(os.path.join(DATA, "data2.vcf"), "rb").read().split(b"\n")
    hdr = [l for l in lines if l.startswith(b"#")]
    recs = [l for l in lines if l and not l.startswith(b"#")]
    head = b"\n".join(hdr + recs[:2]) + b"\n"
    rest = b"\n".join(recs[2:]) + b"\n"
    good = ic.wrap(ic.deflate(head), head)
    broken = bytearray(ic.wrap(ic.deflate(rest), rest)); broken[-6] ^= 0x40
    path = str(tmp_path / "in.vcf.gz")
    open(path, "wb").write(good + bytes(broken) + ic.EOF)
    argv = ["--seed", "1", "--depth", "2", "-e", "0.01", "-O", "v", "-addPL", "1", "--verbose", "1"]
    res = {k: run(["-i", path, "-o", str(tmp_path / ("o" + k)), "--device-inflate", k] + argv, ok=False) for k in ("0", "1")}
    assert res["0"].returncode == res["1"].returncode and res["0"].stdout == res["1"].stdout
    fa = sorted(f[2:] for f in os.listdir(str(tmp_path)) if f.startswith("o0") and not f.endswith(".arg"))
    fb = sorted(f[2:] for f in os.listdir(str(tmp_path)) if f.startswith("o1") and not f.endswith(".arg"))
    assert fa == fb
    for ext in fa:
        assert tci.payload(str(tmp_path / ("o0" + ext))) == tci.payload(str(tmp_path / ("o1" + ext))), ext
    m = FELL_BACK.search(res["1"].stderr)
    if res["1"].returncode == 0:
        assert m and int(m.group(1)) == 3 and "VGL_INFLATE_HOST" in m.group(2), res["1"].stderr[-1500:]
