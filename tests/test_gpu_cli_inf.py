"""vcfgl_hip --depth inf --device-inf 1 (the records made on the device, through the tile ring and every --device-* path) against
--device-inf 0 (one host thread, value by value) of the same build: -O v and -O u files byte for byte, -O z and -O b after
decompression with every BGZF member and the EOF marker checked, the truth files likewise -- all but the header's `##source=` lines,
which hold each run's own command line.  Inputs: data3 with the flag line of the reference's test4 (also against its golden files),
the multi-allelic data5 under every -doUnobserved, and a generated 131-sample x 300-record file with gaps to explode and ties."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bcf_reader
import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(gu.REFVCF, "data", "data3.vcf")
DATA5 = os.path.join(gu.REFVCF, "data", "data5_acgt_multiallelic.vcf")
TEST4 = os.path.join(gu.REFVCF, "reference", "test4")
# runTests.sh, test4 (without its --output-mode)
TEST4_FLAGS = ["--seed", "42", "--depth", "inf", "--error-rate", "0", "--gl-model", "1", "--precise-gl", "0", "-explode", "1", "--rm-empty-sites", "1",
               "--adjust-qs", "1", "-doUnobserved", "1", "-printTruth", "1", "-addGP", "1", "-addPL", "1", "-addI16", "0", "-addQS", "0", "-addFormatDP", "0"]
EXT = {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}
# (output mode, what goes with --device-inf 1)
PATHS = {
    "arrays-v": ("v", []), "arrays-u": ("u", []), "arrays-z": ("z", []), "arrays-b": ("b", []),
    "text-v": ("v", ["--device-text", "1"]), "text-z": ("z", ["--device-text", "1"]),
    "bcf-u": ("u", ["--device-bcf", "1"]), "bcf-b": ("b", ["--device-bcf", "1"]),
    "text-stream": ("z", ["--device-text", "1", "--device-stream", "1", "--device-bgzf", "1"]),
    "bcf-stream": ("b", ["--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]),
    "devices-v": ("v", ["--devices", "0,0"]), "devices-bcf-stream": ("b", ["--devices", "0,0", "--device-bcf", "1", "--device-stream", "1"]),
    "input-v": ("v", ["--device-input", "1"]), "input-text-z": ("z", ["--device-input", "1", "--device-text", "1", "--encode-threads", "3"]),
}


def run(inp, out, mode, *flags, ok=True):
    r = subprocess.run([BIN, "-i", inp, "-o", out, "-O", mode] + list(flags), capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def members(path):
    """every BGZF member of the file: header fields, CRC and sizes checked, the EOF member last and only there"""
    blocks = bcf_reader.bgzf_blocks(open(path, "rb").read())
    assert blocks[-1] == b"" and all(len(b) > 0 for b in blocks[:-1])
    return blocks


def content(path, mode):
    """what the file holds, without the `##source=` lines: text lines, or (BCF header lines, the records' bytes)"""
    if mode in "zb":
        members(path)
    if mode in "vz":
        data = gzip.open(path, "rb").read() if mode == "z" else open(path, "rb").read()
        return [ln for ln in data.decode().split("\n") if not ln.startswith("##source=")]
    r = bcf_reader.Reader(path)
    return [h for h in r.header if not h.startswith("##source=")], bytes(r.raw[r.off:])


def summary(r):
    return r.stderr[r.stderr.index("-> Simulation finished"):]


class Baselines:
    """--device-inf 0 of an input and flag line, per output mode: made on first use, shared"""

    def __init__(self, d):
        self.d, self.made = d, {}

    def get(self, key, inp, mode, flags):
        k = (key, mode)
        if k not in self.made:
            out = str(self.d / ("host_%s_%s" % (key, mode)))
            r = run(inp, out, mode, "--device-inf", "0", *flags)
            truth = content(out + ".truth" + EXT[mode], mode) if "-printTruth" in flags else None
            self.made[k] = (content(out + EXT[mode], mode), truth, summary(r))
        return self.made[k]


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return Baselines(tmp_path_factory.mktemp("inf_cli_host"))


def assert_same_as_host(base, key, inp, mode, flags, extra, tmp_path):
    want, want_truth, want_summary = base.get(key, inp, mode, flags)
    out = str(tmp_path / "dev")
    r = run(inp, out, mode, "--device-inf", "1", *extra, *flags)
    got = content(out + EXT[mode], mode)
    assert got == want, (key, mode, extra)
    if want_truth is not None:
        assert content(out + ".truth" + EXT[mode], mode) == want_truth
    assert summary(r) == want_summary                             # the block run_depth_inf writes
    return got


@pytest.mark.parametrize("tile", ["7", "64"])
@pytest.mark.parametrize("path", ["arrays-v", "text-v", "text-z", "arrays-u", "bcf-b", "text-stream", "devices-v", "input-v"])
def test_data3_with_the_flags_of_test4(base, path, tile, tmp_path):
    mode, extra = PATHS[path]
    got = assert_same_as_host(base, "test4", DATA3, mode, TEST4_FLAGS, extra + ["--tile-sites", tile], tmp_path)
    if mode in "vz":                                              # and the reference's own files, as text
        records = lambda lines: [ln for ln in lines if ln and not ln.startswith("##")]
        assert records(got) == records(open(os.path.join(TEST4, "test4.vcf")).read().split("\n"))
        truth = content(str(tmp_path / "dev") + ".truth" + EXT[mode], mode)
        assert records(truth) == records(open(os.path.join(TEST4, "test4.truth.vcf")).read().split("\n"))


@pytest.mark.parametrize("d", ["0", "1", "2", "3", "4", "5"])
def test_data5_under_every_do_unobserved(base, d, tmp_path):
    flags = ["--seed", "1", "-d", "inf", "-e", "0.01", "--source", "1", "-doUnobserved", d, "-addGP", "1", "-addPL", "1", "-printTruth", "1"]
    for k, path in enumerate(("arrays-v", "text-v", "arrays-u", "bcf-u", "bcf-stream", "text-stream")):
        mode, extra = PATHS[path]
        sub = tmp_path / str(k)
        sub.mkdir()
        got = assert_same_as_host(base, "data5_" + d, DATA5, mode, flags, extra + ["--tile-sites", "4"], sub)
        if path == "arrays-v":
            first = next(ln for ln in got if ln.startswith("chr22\t2\t")).split("\t")
            assert (first[3], first[4].split(",")[:2]) == ("G", ["T", "C"])            # G and T tie at 3: G first


def write_big_vcf(path, n_samples=131, n_records=300, length=400, seed=5):
    """records with all four alleles in a random order, at 300 of 400 positions (gaps to explode, a tail behind the last record); the
    bases of a site follow count patterns with two-, three- and four-way ties, one allele only, rare alleles; hets in both orders"""
    rng = np.random.default_rng(seed)
    M = 2 * n_samples
    k3 = (M - 1) // 3
    patterns = [[M, 0, 0, 0], [M - 1, 1, 0, 0], [M - 2, 1, 1, 0], [M - 3, 1, 1, 1], [M // 2, M // 2, 0, 0], [M - 3 * k3, k3, k3, k3],
                [M // 4, M // 4, M // 4, M - 3 * (M // 4)], [M // 3, M // 3, M - 2 * (M // 3), 0], [M // 4 + 1, M // 4 + 1, M // 4, M - 3 * (M // 4) - 2]]
    pos = np.sort(rng.choice(np.arange(3, length - 5), n_records, replace=False))
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n##contig=<ID=chr1,length=%d>\n" % length)
        f.write("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % s for s in range(n_samples)) + "\n")
        for i, p in enumerate(pos):
            c = patterns[i % 12] if i % 12 < len(patterns) else list(rng.multinomial(M, rng.dirichlet(np.ones(4) * 0.5)))
            order = rng.permutation(4)                                                 # allele index k of the record is base order[k]
            idx = np.repeat(rng.permutation(4), c)                                     # (the pattern's counts fall on the allele indices in a random order)
            rng.shuffle(idx)
            names = ["ACGT"[b] for b in order]
            gts = "\t".join("%d|%d" % (a, b) for a, b in zip(idx[0::2], idx[1::2]))
            f.write("chr1\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (p, names[0], ",".join(names[1:]), gts))
    return path


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return write_big_vcf(str(tmp_path_factory.mktemp("inf_cli_big") / "big.vcf"))


BIG_FLAGS = ["--seed", "3", "-d", "inf", "-e", "0.01", "--source", "1", "-explode", "1", "-doUnobserved", "1", "-addGP", "1", "-addPL", "1", "-printTruth", "1"]


@pytest.mark.parametrize("tile", ["7", "64"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_a_generated_file_with_gaps_and_ties(base, big, path, tile, tmp_path):
    mode, extra = PATHS[path]
    got = assert_same_as_host(base, "big", big, mode, BIG_FLAGS, extra + ["--tile-sites", tile], tmp_path)
    if path == "arrays-v":
        recs = [ln.split("\t") for ln in got if ln and not ln.startswith("#")]
        assert len(recs) == 400 and len(recs[0]) == 9 + 131
        assert {len(r[4].split(",")) for r in recs} == {1, 2, 3, 4}                    # one to four observed alleles, plus <*>
        assert sum(1 for r in recs if r[1] not in {x[1] for x in (ln.split("\t") for ln in open(big) if not ln.startswith("#"))}) == 100


def test_other_tag_sets_and_site_filters(base, big, tmp_path):
    """GL alone, PL alone, GP with the unobserved allele spelled <NON_REF>, all four bases in every record; --rm-invar-sites on the
    host's site stream; the simulation flags the host path ignores"""
    cases = [(["-addGL", "1"], "text-v"), (["-addGL", "0", "-addPL", "1"], "bcf-u"), (["-addGL", "0", "-addGP", "1", "-doUnobserved", "2"], "arrays-v"),
             (["-addPL", "1", "-doUnobserved", "5", "--rm-invar-sites", "3"], "text-stream"), (["-addGP", "1", "-doUnobserved", "3", "--rm-invar-sites", "1"], "bcf-stream"),
             (["-addPL", "1", "--gl-model", "1", "--error-qs", "2", "--beta-variance", "1e-5", "--rng-mode", "1", "--rm-empty-sites", "1", "-addFormatAD", "1",
               "-addInfoDP", "1", "-printBasePickError", "1"], "arrays-u")]
    for k, (tags, path) in enumerate(cases):
        mode, extra = PATHS[path]
        sub = tmp_path / str(k)
        sub.mkdir()
        flags = ["--seed", "3", "-d", "inf", "-e", "0.01", "--source", "1"] + tags
        assert_same_as_host(base, "tags%d" % k, big, mode, flags, extra + ["--tile-sites", "64"], sub)


def test_a_missing_allele_ends_the_run_with_the_hosts_message(tmp_path):
    lines = open(DATA5).read().split("\n")
    recs = [i for i, ln in enumerate(lines) if ln and not ln.startswith("#")]
    for k, gt in ((2, ".|0"), (4, "1|.")):                                             # positions 4 and 6, two tiles apart at --tile-sites 1
        c = lines[recs[k]].split("\t")
        c[-1] = gt
        lines[recs[k]] = "\t".join(c)
    inp = str(tmp_path / "missing.vcf")
    open(inp, "w").write("\n".join(lines))
    flags = ["--seed", "1", "-d", "inf", "-e", "0.01", "--source", "1", "-addPL", "1"]
    want = "--depth inf needs complete A/C/G/T genotypes (position 4)"
    for k, extra in enumerate((["--device-inf", "0"], ["--device-inf", "1"], ["--device-inf", "1", "--tile-sites", "1", "--devices", "0,0"],
                               ["--device-inf", "1", "--tile-sites", "2", "--device-text", "1"])):
        r = run(inp, str(tmp_path / ("o%d" % k)), "v", *extra, *flags, ok=False)
        assert r.returncode == 1 and want in r.stderr and "Simulation finished" not in r.stderr, (extra, r.stderr[-600:])
