"""vcfgl_hip --device-bcf 1 (the FORMAT part of -O u / -O b records encoded on the device) writes the files --device-bcf 0 writes: over
the flag matrix of tests/test_gpu_cli_vcftext.py in every binary mode, with a record of 15 values per sample among them; gVCF runs with
--device-gvcf 1 --device-bcf 1 against the host blocker in the same -O mode (blocks that cross tiles; five-allele sites); and
the reference's golden configurations again, decoded by tests/bcf_reader.py."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bcf_reader
import golden_util as gu
import test_gpu_cli as tcli
import test_gpu_cli_gvcf as tcg
import test_gpu_cli_vcftext as tcv

pytestmark = pytest.mark.gpu
BIN = tcv.BIN
DATA = tcv.DATA
MODES = {"u": ("u", []), "b": ("b", []), "b-threads": ("b", ["--threads", "16"]), "b-bgzf": ("b", ["--device-bgzf", "1"]),
         "u-devices": ("u", ["--devices", "0,0"])}


def stream(path):
    """(header lines without ##source=, record bytes) of a BCF file, decompressed when it is BGZF"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = b"".join(bcf_reader.bgzf_blocks(raw))
    assert raw[:5] == b"BCF\x02\x02"
    l_text = struct.unpack_from("<I", raw, 5)[0]
    header = [l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")]
    return header, raw[9 + l_text:]


def run(out, mode, flags, extra=()):
    r = subprocess.run([BIN, "-o", out, "-O", mode, "--seed", "42", "--tile-sites", "7"] + list(extra) + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def same_outputs(a, b, ra, rb):
    ha, da = stream(a + ".bcf")
    hb, db = stream(b + ".bcf")
    assert ha == hb
    assert da == db
    assert ra.stdout == rb.stdout                                  # per-read listings
    if os.path.exists(a + ".pileup.gz"):
        assert gzip.open(a + ".pileup.gz").read() == gzip.open(b + ".pileup.gz").read()
    assert os.path.exists(a + ".truth.bcf") == os.path.exists(b + ".truth.bcf")
    if os.path.exists(a + ".truth.bcf"):
        assert stream(a + ".truth.bcf") == stream(b + ".truth.bcf")
    return da


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", sorted(tcv.CASES))
def test_device_bcf_equals_host_bcf(case, mode, tmp_path):
    m, extra = MODES[mode]
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = run(a, m, tcv.CASES[case], extra + ["--device-bcf", "0"])
    rb = run(b, m, tcv.CASES[case], extra + ["--device-bcf", "1"])
    assert len(same_outputs(a, b, ra, rb)) > 100
    if case in ("alltags", "pileup"):
        assert os.path.exists(a + (".truth.bcf" if case == "alltags" else ".pileup.gz"))


def test_a_record_of_fifteen_values_per_sample(tmp_path):
    """-doUnobserved 4 with -explode 1: A, C, G, T and <*> -- five alleles, 15 PL / GL / GP values per sample (the size byte 0xF.
    followed by a typed 15); the --device-bcf 0 run itself shows it, and the device writes the same bytes"""
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = run(a, "u", tcv.CASES["eq2precise"], ["--device-bcf", "0"])
    rb = run(b, "u", tcv.CASES["eq2precise"], ["--device-bcf", "1"])
    same_outputs(a, b, ra, rb)
    for path in (a, b):
        recs = list(bcf_reader.Reader(path + ".bcf").records())
        wide = [r for r in recs if len(r["alleles"]) == 5]
        assert wide
        for r in wide:
            per = {k: len(v[0]) for k, _, v in r["fmt"]}
            assert per["PL"] == per["GL"] == per["GP"] == 15 and per["AD"] == 5 and per["DP"] == 1


GVCF_MODES = {"v": ("u", []), "z": ("b", []), "z-bgzf": ("b", ["--device-bgzf", "1"])}


@pytest.mark.parametrize("case", range(len(tcg.CASES)))
def test_random_gvcf_runs_equal_the_host_blocker(case, tmp_path):
    """the shapes of tests/test_gpu_cli_gvcf.py (tile sizes 7 and 64 make blocks cross tiles) in -O u / -O b: the host blocker, whose
    blocks go through the text round trip, against --device-gvcf 1 --device-bcf 1"""
    c = tcg.CASES[case]
    rng = np.random.default_rng(c["seed"])
    inp = str(tmp_path / "in.vcf")
    tcg.random_vcf(rng, inp, c["N"], contigs=int(rng.integers(1, 4)))
    depth = 2.0 if c["pileup"] else 12.0 if c["N"] >= 65 else float(rng.choice([3.0, 12.0]))
    dps = sorted({1} | set(int(x) for x in rng.integers(2, 12, int(rng.integers(0, 4)))))
    err = 0.0 if c["N"] >= 65 else float(rng.choice([0.0, 0.001]))
    m, extra = GVCF_MODES[c["mode"]]
    argv = ["-i", inp, "-O", m, "--seed", str(c["seed"]), "--depth", str(depth), "--error-rate", str(err),
            "-explode", "1", "-doUnobserved", str(int(rng.choice([1, 2]))), "-addPL", "1", "-doGVCF", "1", "--gvcf-dps", ",".join(map(str, dps)),
            "--tile-sites", str(c["tile"]), "-addQS", str(int(c["qs"])), "--rm-empty-sites", str(int(c["rm_empty"])),
            "-printPileup", str(int(c["pileup"]))] + extra
    if c["devices"]:
        argv += ["--devices", "0,0"]
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = tcg.run(argv + ["-o", a])
    rb = tcg.run(argv + ["-o", b, "--device-gvcf", "1", "--device-bcf", "1"])
    same_outputs(a, b, ra, rb)
    recs = list(bcf_reader.Reader(b + ".bcf").records())
    assert len(recs) > 8 and any(k == "MIN_DP" for r in recs for k, _, _ in r["info"])
    assert any([k for k, _, _ in r["fmt"]] == ["PL", "DP"] for r in recs)            # blocks
    assert "Number of sites included" in rb.stderr


@pytest.mark.parametrize("tile", [3, 4096])
def test_five_allele_sites_never_block_and_both_paths_agree(tile, tmp_path):
    """The fatal "Unexpected number of PL values" needs a blockable site (exactly one observed allele) whose record has other than two
    alleles.  The command line cannot produce one: -doGVCF 1 accepts -doUnobserved 1 / 2 (one observed allele gives exactly two alleles)
    and 4 / 5 (A, C, G and T all count as observed: four observed alleles, never blockable), so the message is reachable through the
    library only, where tests/test_gpu_gvcf.py::test_five_allele_founder_alone_and_joined pins the reported site and write_gvcf_tile
    turns it into the host blocker's message.  What can be run is run here: hom-ref sites of five alleles, inside a tile and (tile size
    3) across tiles -- both paths end the same way, without the message, with the same bytes, every site a record of 15 PL values."""
    inp = str(tmp_path / "in.vcf")
    with open(inp, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=20>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts0\ts1\n")
        for p in range(1, 9):
            fh.write(f"chr1\t{p}\t.\t0\t1\t.\tPASS\t.\tGT\t0|0\t0|0\n")
    argv = ["-i", inp, "-O", "u", "--seed", "5", "--depth", "12", "--error-rate", "0", "-explode", "1", "-doUnobserved", "4", "-addPL", "1",
            "-doGVCF", "1", "--gvcf-dps", "1", "--tile-sites", str(tile)]
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = subprocess.run([BIN] + argv + ["-o", a], capture_output=True, text=True, timeout=300)
    rb = subprocess.run([BIN] + argv + ["-o", b, "--device-gvcf", "1", "--device-bcf", "1"], capture_output=True, text=True, timeout=300)
    assert ra.returncode == rb.returncode == 0, (ra.stderr[-500:], rb.stderr[-500:])
    assert "Unexpected number of PL values" not in ra.stderr + rb.stderr
    same_outputs(a, b, ra, rb)
    recs = list(bcf_reader.Reader(b + ".bcf").records())
    assert len(recs) == 20 and all(len(r["alleles"]) == 5 and [len(v[0]) for k, _, v in r["fmt"] if k == "PL"] == [15] for r in recs)


# the golden configuration the flag refuses (--depth inf: no tile is simulated); it is not run here
REFUSED_GOLD = ["test4"]
GOLD = [n for n in sorted(gu.REF_TESTS, key=lambda s: int(s[4:])) if n not in REFUSED_GOLD]


@pytest.mark.parametrize("name", GOLD)
def test_golden_outputs_with_device_bcf(name, tmp_path):
    t = gu.REF_TESTS[name]
    argv, toks = [], t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        if flag in ("--output-mode", "-O"):
            val = "u"
        argv += [flag, val]
    assert "inf" not in argv and len(GOLD) == len(gu.REF_TESTS) - sum(n in gu.REF_TESTS for n in REFUSED_GOLD)
    if "-doGVCF 1" in t["args"]:
        argv += ["--device-gvcf", "1"]
    out = str(tmp_path / name)
    r = subprocess.run([BIN, "-i", os.path.join(DATA, t["input"]), "-o", out, "--rng-mode", "1", "--device-bcf", "1"] + argv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ft = tcli._FloatText()
    rd = bcf_reader.Reader(out + ".bcf")
    assert not rd.compressed
    bits = []
    for rec in rd.records():
        bits += [x for _, ty, v in rec["info"] if ty == 5 for x in v]
        bits += [x for _, ty, per in rec["fmt"] if ty == 5 for v in per for x in v]
    ft.prime(bits)
    ours = list(bcf_reader.Reader(out + ".bcf").vcf_lines(ft))
    gold = [l.rstrip("\n") for l in open(os.path.join(gu.REFVCF, "reference", name, name + ".vcf")) if not l.startswith("#")]
    assert ours == gold


def test_a_run_without_a_visible_gpu_fails_and_does_not_fall_back(tmp_path):
    """the child process sees no device: the run with the flag ends with the library's message and exit code 1"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = str(tmp_path / "o")
    r = subprocess.run([BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "-O", "u", "--seed", "1", "-e", "0.01", "--depth", "2", "--device-bcf", "1"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert "[ERROR]" in r.stderr and "device" in r.stderr.lower()
    assert "Simulation finished successfully" not in r.stderr
