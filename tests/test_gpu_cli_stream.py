"""vcfgl_hip --device-stream 1 (a tile's records assembled and BGZF-compressed on the device that simulated it) writes files that
decompress to what --device-stream 0 writes: over the flag matrix of tests/test_gpu_cli_vcftext.py for -O b --device-bcf 1 and
-O z --device-text 1, with the BGZF streams of the run compressed on the host and on the device and over two contexts; the member
boundaries restart at every tile; and the reference's golden configurations again, decoded by tests/bcf_reader.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bcf_reader
import bgzf_model
import golden_util as gu
import test_gpu_cli as tcli
import test_gpu_cli_bcf as tcb
import test_gpu_cli_gvcf as tcg
import test_gpu_cli_vcftext as tcv

pytestmark = pytest.mark.gpu
BIN = tcv.BIN
DATA = tcv.DATA
M = bgzf_model.MEMBER
OUTPUTS = {"b": ("b", ".bcf", ["--device-bcf", "1"]), "z": ("z", ".vcf.gz", ["--device-text", "1"])}
MODES = {"host-bgzf": ["--device-bgzf", "0"], "device-bgzf": ["--device-bgzf", "1"], "devices": ["--devices", "0,0"]}


def members(path):
    """payload of every BGZF member of the file; header fields, CRC and sizes checked, the EOF member last and only there"""
    raw = open(path, "rb").read()
    blocks = bcf_reader.bgzf_blocks(raw)                              # (asserts the last 28 bytes are the EOF member)
    assert blocks[-1] == b"" and all(len(b) > 0 for b in blocks[:-1])
    return blocks


def same_files(a, b, ext, ra, rb):
    ma, mb = members(a + ext), members(b + ext)
    if ext == ".bcf":
        tcb.same_outputs(a, b, ra, rb)                                # header, record bytes, stdout, pileup, truth file
    else:
        assert tcv.body(a + ext) == tcv.body(b + ext) and len(tcv.body(a + ext)) > 10
        assert ra.stdout == rb.stdout                                 # per-read listings
        if os.path.exists(a + ".pileup.gz"):
            assert gzip.open(a + ".pileup.gz").read() == gzip.open(b + ".pileup.gz").read()
        assert os.path.exists(a + ".truth" + ext) == os.path.exists(b + ".truth" + ext)
        if os.path.exists(a + ".truth" + ext):
            assert tcv.body(a + ".truth" + ext) == tcv.body(b + ".truth" + ext)
    return ma, mb


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("output", sorted(OUTPUTS))
@pytest.mark.parametrize("case", sorted(tcv.CASES))
def test_device_stream_equals_host_stream(case, output, mode, tmp_path):
    m, ext, companion = OUTPUTS[output]
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = tcv.run(a, m, tcv.CASES[case], companion + MODES[mode] + ["--device-stream", "0"])
    rb = tcv.run(b, m, tcv.CASES[case], companion + MODES[mode] + ["--device-stream", "1"])
    ma, mb = same_files(a, b, ext, ra, rb)
    assert len(mb) > len(ma)                                          # tiles of 7 sites: a member (at least) per tile
    if case in ("alltags", "pileup"):
        assert os.path.exists(b + (".truth" + ext if case == "alltags" else ".pileup.gz"))


@pytest.mark.parametrize("output", sorted(OUTPUTS))
def test_member_boundaries_restart_at_every_tile(output, tmp_path):
    """about 300 samples at --tile-sites 64: a tile's records take several members.  With --device-stream 0 every member but the last
    holds 0xff00 bytes; with --device-stream 1 the header's member and every tile's last member are shorter, wherever they lie"""
    m, ext, companion = OUTPUTS[output]
    rng = np.random.default_rng(77)
    inp = str(tmp_path / "in.vcf")
    tcg.random_vcf(rng, inp, 300, contigs=3)
    argv = ["-i", inp, "-O", m, "--seed", "9", "--depth", "4", "--error-rate", "0.01", "-explode", "1", "-addPL", "1", "--tile-sites", "64"] + companion
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = tcg.run(argv + ["-o", a, "--device-stream", "0"])
    rb = tcg.run(argv + ["-o", b, "--device-stream", "1"])
    ma, mb = same_files(a, b, ext, ra, rb)                            # equal decompressed bytes, but for ##source=
    assert all(len(x) == M for x in ma[:-2]) and len(ma) > 4          # one stream: full members up to the last data member
    sizes = [len(x) for x in mb[:-1]]                                 # data members (without the EOF member)
    n_sites = int(rb.stderr.split("Total number of sites simulated:")[1].split()[0])
    assert n_sites > 2 * 64
    # behind the header's member the stream is tiles: runs of full members, each closed by a shorter one
    tiles, run = [], 0
    for s in sizes[1:]:
        run += 1
        if s < M:
            tiles.append(run)
            run = 0
    assert run == 0 and len(tiles) == -(-n_sites // 64)               # every tile ends its own members
    assert max(tiles) >= 2                                            # some tile produced at least two members
    assert any(s < M for s in sizes[1:-1])                            # a short member in front of the last data member


# the golden configurations the flag refuses: --depth inf (no tile is simulated) and -doGVCF 1 (blocks are emitted by the host)
GOLD = [n for n in sorted(gu.REF_TESTS, key=lambda s: int(s[4:])) if "inf" not in gu.REF_TESTS[n]["args"].split() and "-doGVCF 1" not in gu.REF_TESTS[n]["args"]]


@pytest.mark.parametrize("name", GOLD)
def test_golden_outputs_with_device_stream(name, tmp_path):
    t = gu.REF_TESTS[name]
    argv, toks = [], t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        if flag in ("--output-mode", "-O"):
            continue
        argv += [flag, val]
    assert 0 < len(GOLD) < len(gu.REF_TESTS) and "test4" not in GOLD
    out = str(tmp_path / name)
    r = subprocess.run([BIN, "-i", os.path.join(DATA, t["input"]), "-o", out, "--rng-mode", "1", "-O", "b", "--device-bcf", "1", "--device-stream", "1"] + argv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    members(out + ".bcf")
    ft = tcli._FloatText()
    rd = bcf_reader.Reader(out + ".bcf")
    assert rd.compressed
    bits = []
    for rec in rd.records():
        bits += [x for _, ty, v in rec["info"] if ty == 5 for x in v]
        bits += [x for _, ty, per in rec["fmt"] if ty == 5 for v in per for x in v]
    ft.prime(bits)
    ours = list(bcf_reader.Reader(out + ".bcf").vcf_lines(ft))
    gold = [l.rstrip("\n") for l in open(os.path.join(gu.REFVCF, "reference", name, name + ".vcf")) if not l.startswith("#")]
    assert ours == gold


def test_verbose_line_counts_the_members_that_came_back(tmp_path):
    """--verbose 1: the per-device line of the mode reports heads up and members down; the members are (most of) the file"""
    a = str(tmp_path / "o")
    r = tcv.run(a, "b", tcv.CASES["gl1"], ["--device-bcf", "1", "--device-stream", "1", "--verbose", "1"])
    assert "--device-stream 1:" in r.stderr and "GB of BGZF members copied back" in r.stderr and "[timing] read input" in r.stderr
    size = os.path.getsize(a + ".bcf")
    down = float(r.stderr.split("sent up, ")[1].split(" GB of BGZF members")[0]) * 1e9
    assert 0 < down <= size
