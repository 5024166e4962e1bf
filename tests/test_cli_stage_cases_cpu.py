"""The generator and the comparer of the device-stage differential test (tests/cli_stage_cases.py), without a GPU: draw() is
deterministic per seed; the fixed seeds of tests/test_gpu_cli_stages_fuzz.py (18000 + chunk, chunks 0-15, six cases each) reach every
stage flag, output mode, input container, sample count and the rarer kinds of run as often as that test relies on; the host twin keeps
what defines output and nothing else; the comparer reports one differing byte, a missing file and another exit status; and the CPU
oracle refuses few enough of the drawn reference flags for the GPU test to spend its processes on runs that run.

Refusals over the 96 fixed configurations (either RNG mode; --depth inf, which the oracle does not know, counted as running):
2 of 96 -- both draw a quality score of 76 with a --qs-bins file that ends at 63.  (On an MI355X the same two are refused, by the
device run and by its host twin with the same message, in both RNG modes.)"""
import collections
import dataclasses
import gzip
import os

import numpy as np
import pytest

import cli_stage_cases as sc
from vcfgl_amd import _abi
from vcfgl_amd.recordloop import iter_sites
from vcfgl_amd.vcfio import read_vcf


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_cases")
    return [c for chunk in range(sc.CHUNKS) for c in sc.fixed_cases(chunk, d)]


def test_draw_is_deterministic_per_seed(tmp_path):
    for seed in (sc.SEED, sc.SEED + 7, 5):
        a = [sc.draw(np.random.default_rng(seed), tmp_path / ("a%d" % seed)) for _ in range(1)]
        b = [sc.draw(np.random.default_rng(seed), tmp_path / ("b%d" % seed)) for _ in range(1)]
        for x, y in zip(a, b):
            strip = lambda c, d: [str(v).replace(str(d), "") for v in dataclasses.astuple(c)]
            assert strip(x, tmp_path / ("a%d" % seed)) == strip(y, tmp_path / ("b%d" % seed))
            assert open(x.input, "rb").read() == open(y.input, "rb").read()
            for fn in ("depths.txt", "bins.csv", "alleles.tsv"):
                pa, pb = os.path.join(os.path.dirname(x.input), fn), os.path.join(os.path.dirname(y.input), fn)
                assert os.path.exists(pa) == os.path.exists(pb) and (not os.path.exists(pa) or open(pa).read() == open(pb).read())
    assert sc.draw(np.random.default_rng(1), tmp_path / "p").ref_flags != sc.draw(np.random.default_rng(2), tmp_path / "q").ref_flags


def test_the_fixed_seeds_reach_every_stage_mode_container_and_shape(cases):
    assert len(cases) == 96
    n = collections.Counter()
    for c in cases:
        n.update(c.stages())
        n.update(["O:" + c.mode, "in:" + c.container, "N:%d" % c.n_samples, "kind:" + c.kind])
        n.update(k for k in ("--set-alleles", "--fetch-gl", "--gt-discordance") if c.has(k, None))
        n["--records 0"] += c.records0
        n["one-site tiles on three contexts"] += c.shape_flags[:4] == ["--tile-sites", "1", "--devices", "0,0,0"]
    for key in list(sc.STAGES) + ["O:" + m for m in sc.MODES] + ["in:" + k for k in sc.CONTAINERS]:
        assert n[key] >= 6, (key, n[key])
    for key in ("kind:gvcf", "kind:inf", "--set-alleles", "--fetch-gl", "--records 0"):
        assert n[key] >= 4, (key, n[key])
    for N in sc.SAMPLE_COUNTS:
        assert n["N:%d" % N] >= 1, N
    assert n["one-site tiles on three contexts"] >= 1
    # the situations no hand-picked flag set of the per-stage tests holds
    three = [c for c in cases if c.shape_flags[:4] == ["--tile-sites", "1", "--devices", "0,0,0"]]
    assert {65, 257} <= {c.n_samples for c in three}
    assert any(c.has("--set-alleles", None) and "--device-stream" in c.stages() for c in cases)
    assert any(c.has("-doUnobserved", "3") and c.stages() for c in cases)
    assert any(c.has("--rm-invar-sites", "2") and c.has("--rm-empty-sites", "1") for c in cases)
    assert any("--depths-file" in c.ref_flags and "0.0" in open(c.ref_flags[c.ref_flags.index("--depths-file") + 1]).read().split() for c in cases)
    assert any(c.has("-addGL", "0") and c.stages() for c in cases)
    assert all(1 <= c.n_records <= 40 and c.n_sites <= 200 for c in cases)
    assert max(c.n_sites for c in cases) > 100 and min(c.n_records for c in cases) <= 2


def test_every_container_holds_the_records_of_the_plain_text(cases):
    """the BGZF containers inflate to the plain ones, and the BCF's genotypes, alleles, contigs and positions are the text's"""
    import bcf_reader
    seen = set()
    for c in cases[:24]:
        seen.add(c.container)
        raw = open(c.input, "rb").read()
        if c.container in ("vcf.gz", "bgzf.bcf"):
            assert raw[:4] == b"\x1f\x8b\x08\x04" and raw.endswith(sc.ic.EOF)
            raw = gzip.decompress(raw)
        if "bcf" not in c.container:
            assert raw == open(c.vcf, "rb").read()
            continue
        assert raw == sc.bcf_of(read_vcf(c.vcf))
        vcf = read_vcf(c.vcf)
        recs = list(bcf_reader.Reader(c.input).records())
        assert len(recs) == len(vcf.records) == c.n_records
        for got, want in zip(recs, vcf.records):
            assert (got["chrom"], got["pos0"], got["alleles"]) == (want.chrom, want.pos0, want.alleles)
            gt = next(per for k, _, per in got["fmt"] if k == "GT")
            assert [((v[0] >> 1) - 1, (v[1] >> 1) - 1) for v in gt] == list(want.gts)
            assert ["|" if v[1] & 1 else "/" for v in gt] == ["|" if "|" in s["GT"][0] else "/" for s in want.samples]
    assert seen == set(sc.CONTAINERS)


def test_the_table_admits_what_it_draws_and_the_twin_keeps_only_what_defines_output(cases):
    for c in cases:
        facts = sc._facts(c.mode, c.kind, c.container, c.ref_flags, c.side_flags) | set(c.stages())
        assert all(sc.STAGES[f](facts) for f in c.stages()), c
        t = sc.host_twin(c)
        assert (t.input, t.mode, t.ref_flags, t.side_flags) == (c.input, c.mode, c.ref_flags, c.side_flags)
        argv = t.argv("o", 0)
        for f in sc.STAGES:
            assert argv[argv.index(f) + 1] == "0"
        assert argv[argv.index("--records") + 1] == "1" and argv[argv.index("--devices") + 1] == "0" and argv[argv.index("--tile-sites") + 1] == "4096"
        serial = c.argv("o", 1)
        assert serial[serial.index("--devices") + 1] == "0" and serial[serial.index("--rng-mode") + 1] == "1"
        if c.has("--set-alleles", None):
            tsv = c.side_flags[c.side_flags.index("--set-alleles") + 1]
            lines = open(tsv).read().splitlines()
            assert len(lines) == c.n_sites and c.has("-doUnobserved", "4")
            for ln in lines:
                ref, alts = ln.split("\t")
                names = [ref] + alts.split(",")
                assert 2 <= len(names) <= 5 and len(set(names)) == len(names) and set(names) <= set(sc.NAMES)


def _write_run(prefix, mode, edit=None):
    """the files of a run with records, truth, pileup, table and CSV; edit(name, bytes) -> bytes or None (no file)"""
    text = b"##fileformat=VCFv4.2\n##source=x\n#CHROM\tPOS\nchr1\t1\n"
    bcf = b"BCF\x02\x02" + (len(text) + 1).to_bytes(4, "little") + text + b"\0" + bytes(range(40))
    body = {"v": text, "z": gzip.compress(text), "u": bcf, "b": sc.ic.bgzf_level6(bcf)}[mode]
    files = {sc.EXT[mode]: body, ".truth" + sc.EXT[mode]: body, ".pileup.gz": gzip.compress(b"chr1\t1\tN\t3\tACG\n"),
             ".discordance.tsv": b"smp0\t1\t2\n", ".fetchgl.csv": b"1,-0.5\n"}
    for ext, data in files.items():
        data = edit(ext, data) if edit else data
        if data is not None:
            open(prefix + ext, "wb").write(data)


@pytest.mark.parametrize("mode", sc.MODES)
def test_the_comparer_reports_one_byte_a_missing_file_and_the_exit_status(mode, tmp_path):
    a = str(tmp_path / "a")
    _write_run(a, mode)
    A = sc.artifacts(a, mode, 0, "line\n", "[timing] 1 s\n")
    assert all(A[k] is not None for k in A if k != "stderr")
    b = str(tmp_path / "same")
    _write_run(b, mode, lambda ext, data: data.replace(b"##source=x", b"##source=another one") if data.startswith(b"##file") else data)
    assert sc.differences(A, sc.artifacts(b, mode, 0, "line\n", "[timing] 2 s\n")) == []
    names = {sc.EXT[mode]: "records", ".truth" + sc.EXT[mode]: "truth", ".pileup.gz": "pileup", ".discordance.tsv": "discordance", ".fetchgl.csv": "fetchgl"}
    for k, (ext, name) in enumerate(names.items()):
        def one_byte(e, data, ext=ext):
            if e != ext:
                return data
            if e.endswith(".gz") or (mode == "b" and e.endswith(".bcf")):            # the last byte of what the container holds
                raw = gzip.decompress(data)
                raw = raw[:-1] + bytes([raw[-1] ^ 1])
                return sc.ic.bgzf_level6(raw) if mode == "b" and e.endswith(".bcf") else gzip.compress(raw)
            return data[:-1] + bytes([data[-1] ^ 1])
        p = str(tmp_path / ("byte%d" % k))
        _write_run(p, mode, one_byte)
        assert sc.differences(A, sc.artifacts(p, mode, 0, "line\n", "")) == [name]
        p = str(tmp_path / ("gone%d" % k))
        _write_run(p, mode, lambda e, data, ext=ext: None if e == ext else data)
        assert sc.differences(A, sc.artifacts(p, mode, 0, "line\n", "")) == [name]
        assert sc.differences(A, sc.artifacts(p, mode, 0, "line\n", ""), skip=(name,)) == []
    assert sc.differences(A, sc.artifacts(a, mode, 1, "line\n", "[ERROR] x\n")) == ["status", "stderr"]
    assert sc.differences(A, sc.artifacts(a, mode, 0, "linf\n", "")) == ["stdout"]
    E = sc.artifacts(a, mode, 1, "", "[input] 5 lines\n\n*******\n[ERROR] a message\n*******\n")
    assert sc.differences(E, sc.artifacts(a, mode, 1, "", "[input] 6 lines\n[timing] 3 s\n\n*******\n[ERROR] a message\n*******\n")) == []
    assert sc.differences(E, sc.artifacts(a, mode, 1, "", "\n*******\n[ERROR] another message\n*******\n")) == ["stderr"]
    # two refused runs: what each had written by then is not compared (the tile size decides it), status and message are
    p = str(tmp_path / "cut")
    _write_run(p, mode, lambda e, data: b"" if e == sc.EXT[mode] else None)
    assert sc.differences(E, sc.artifacts(p, mode, 1, "x", "[timing]\n\n*******\n[ERROR] a message\n*******\n")) == []
    assert sc.differences(E, sc.artifacts(p, mode, 2, "", "\n*******\n[ERROR] a message\n*******\n")) == ["status"]
    # a run that ends well beside an empty record file: a difference, not an exception
    assert sc.differences(A, sc.artifacts(p, mode, 0, "line\n", ""))[:1] == ["records"]


def oracle_refuses(oracle, case):
    """does the CPU oracle refuse the case's reference flags on its sites, in either RNG mode?  (The message, or None.)"""
    if case.kind == "inf":
        return None
    for mode, beta in ((_abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48), (_abi.VGL_RNG_SERIAL, _abi.VGL_BETA_STD)):
        args = sc._oracle_args(case.ref_flags)
        args.rng_mode, args.beta_sampler = mode, beta
        sites = list(iter_sites(read_vcf(case.vcf), args))
        if not sites:
            continue
        fields = [f for f, _, _ in _abi.TILE_FIELDS if not (f == "qs" and not (args.add_qs or args.add_i16)) and not (f == "i16" and not args.add_i16)]
        try:
            oracle.Oracle(args, case.n_samples).simulate(0, np.stack([s.gt for s in sites]), fields=fields)
        except oracle.OracleError as e:
            return "%s (rng mode %d)" % (e, mode)
    return None


def test_at_most_one_configuration_in_ten_is_refused_by_the_oracle(oracle, cases):
    refused = [(k, msg) for k, msg in ((k, oracle_refuses(oracle, c)) for k, c in enumerate(cases)) if msg]
    print("refused by the oracle: %d of %d" % (len(refused), len(cases)), refused)
    assert 10 * len(refused) <= len(cases), refused
