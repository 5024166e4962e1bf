"""vcfgl_hip --device-bgzf 1: every BGZF stream of the run compressed on the GPU.  The decompressed output and pileup equal the
default (host zlib) run's byte for byte, tests/bcf_reader.py reads the file (CRCs, sizes, EOF member), the program reads it back as
input, and the compressed file does not depend on --threads or on the device count."""
import gzip
import os
import subprocess

import pytest

import bcf_reader
import golden_util as gu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")

FLAGS = {
    "plain": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "6", "--error-rate", "0.01", "-explode", "1", "-addPL", "1", "-addGP", "1",
              "-addFormatAD", "1", "-printTruth", "1"],
    "i16qs": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "8", "--error-rate", "0.01", "--error-qs", "2", "--beta-variance", "1e-5",
              "-explode", "1", "-addI16", "1", "-addQS", "1"],
    "gvcf": ["-i", os.path.join(DATA, "data2.vcf"), "--depth", "4", "--error-rate", "0.001", "-explode", "1", "-doUnobserved", "2", "-addPL", "1",
             "-doGVCF", "1", "--gvcf-dps", "1,3"],
    "pileup": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "3", "--error-rate", "0.02", "--error-qs", "2", "--beta-variance", "1e-4",
               "-explode", "1", "-printPileup", "1"],
}
EXT = {"b": ".bcf", "z": ".vcf.gz"}


def run(out, mode, flags, extra=()):
    r = subprocess.run([BIN, "-o", out, "-O", mode, "--seed", "42", "--tile-sites", "3"] + list(extra) + flags,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def inflate(path):
    raw = open(path, "rb").read()
    return b"".join(bcf_reader.bgzf_blocks(raw))      # checks every member's header, CRC, ISIZE and the EOF member


def body(data, mode):
    # the header carries the command line, which differs in --device-bgzf: compare what follows it
    if mode == "z":
        return [l for l in data.split(b"\n") if not l.startswith(b"##")]
    return data[5 + 4 + int.from_bytes(data[5:9], "little"):]


@pytest.mark.parametrize("case", sorted(FLAGS))
@pytest.mark.parametrize("mode", ["b", "z"])
def test_device_bgzf_equals_the_zlib_path(case, mode, tmp_path):
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    run(host, mode, FLAGS[case])
    run(dev, mode, FLAGS[case], ["--device-bgzf", "1"])
    a, b = inflate(host + EXT[mode]), inflate(dev + EXT[mode])
    assert len(a) > 100 and body(a, mode) == body(b, mode)
    assert open(host + EXT[mode], "rb").read() != open(dev + EXT[mode], "rb").read()      # really another compressor
    if case == "pileup":
        assert inflate(host + ".pileup.gz") == inflate(dev + ".pileup.gz")
        assert gzip.open(dev + ".pileup.gz").read() == inflate(host + ".pileup.gz")
    if case == "plain":
        assert body(inflate(host + ".truth" + EXT[mode]), mode) == body(inflate(dev + ".truth" + EXT[mode]), mode)
    if mode == "b":
        fmt = lambda bits: "%08x" % bits
        assert list(bcf_reader.Reader(dev + ".bcf").vcf_lines(fmt)) == list(bcf_reader.Reader(host + ".bcf").vcf_lines(fmt))


def test_reads_its_own_device_compressed_bcf(tmp_path):
    """-printTruth 1 -O b writes the decoded input (with GT) as a BGZF BCF: read back with -i, the device-compressed one gives the
    same run as the zlib-compressed one"""
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    run(host, "b", FLAGS["plain"])
    run(dev, "b", FLAGS["plain"], ["--device-bgzf", "1"])
    rd = bcf_reader.Reader(dev + ".truth.bcf")
    assert rd.compressed
    outs = []
    for src in (host, dev):
        out = src + "_again"
        r = subprocess.run([BIN, "-i", src + ".truth.bcf", "--source", "1", "-o", out, "-O", "v", "--seed", "7", "-d", "4", "-e", "0.01", "-addPL", "1"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append([l for l in open(out + ".vcf") if not l.startswith("##")])
    assert len(outs[0]) > 5 and outs[0] == outs[1]


def test_device_bgzf_file_does_not_depend_on_threads_or_devices(tmp_path):
    """the pileup (no header) byte for byte; the output file's records after decompression (its header holds the command line)"""
    piles, recs = [], []
    for name, extra in (("t1", ["--threads", "1"]), ("t16", ["--threads", "16"]), ("d0", ["--devices", "0"]), ("d00", ["--devices", "0,0"])):
        out = str(tmp_path / name)
        run(out, "b", FLAGS["pileup"] + ["-addI16", "1", "-addQS", "1"], extra + ["--device-bgzf", "1"])
        piles.append(open(out + ".pileup.gz", "rb").read())
        rd = bcf_reader.Reader(out + ".bcf")
        assert rd.compressed
        recs.append(rd.raw[rd.off:])
    assert len(piles[0]) > 100 and all(p == piles[0] for p in piles)
    assert len(recs[0]) > 500 and all(r == recs[0] for r in recs)
