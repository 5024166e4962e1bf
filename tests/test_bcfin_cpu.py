"""The BCF genotype decoder without a GPU: tests/bcfin_model.py (the statement of what the device decoder computes) against the host
program's own reader (vcfgl_hip --dump-gt FILE SOURCE 0) and against the model of the text parser on the same genotypes, the statuses
the shared per-sample rule gives on the host (--dump-gt FILE SOURCE 3), the boundary between plain and handed-back records, the
fallback share of every hand-built input of the GPU tests, the declarations, and the refusals of the flag and of a machine without a
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bcfin_cases as bc
import bcfin_model as bm
import golden_util as gu
import test_vcfin_cpu as tvc
import vcfin_model as vm
from vcfgl_amd import _abi

ROOT = tvc.ROOT
BIN = tvc.BIN
DATA = os.path.join(gu.REFVCF, "data")


def run(argv, ok=True):
    r = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def golden_bcf(path, mode, out_dir):
    """the BCF the program writes from a golden input: the truth file of a --depth inf run keeps GT (raw with -O u, BGZF with -O b).
    A --source 0 input comes back with the alleles A, C, so every such BCF is read with --source 1"""
    src = os.path.join(str(out_dir), os.path.basename(path) + "." + mode)
    run(["-i", path, "-o", src, "--seed", "1", "--depth", "inf", "-e", "0", "-O", mode, "--source", str(tvc._source(path)), "-printTruth", "1"])
    return src + ".truth.bcf"


@pytest.fixture(scope="module")
def golden_bcfs(tmp_path_factory):
    d = tmp_path_factory.mktemp("golden_bcf")
    return {(p, mode): golden_bcf(p, mode, d) for p in tvc.GOLDEN for mode in ("u", "b")}


def dump(path, source, mode):
    r = run(["--dump-gt", path, str(source), str(mode)])
    return r.stdout


@pytest.mark.parametrize("mode", ["u", "b"])
@pytest.mark.parametrize("path", tvc.GOLDEN, ids=tvc.IDS)
def test_model_equals_the_host_reader_on_the_golden_inputs(path, mode, golden_bcfs):
    bcf = golden_bcfs[(path, mode)]
    raw = bm.read_raw(bcf)
    assert raw[:3] == b"BCF" and (open(bcf, "rb").read(2) == b"\x1f\x8b") == (mode == "b")
    rows = bm.file_rows(raw, 1)
    assert len(rows) == len(vm.read_lines(path)[2]) > 0
    assert dump(bcf, 1, 0) == bm.dump_text(rows, status=-1)            # today's read_bcf + make_site: a BCF record has no status there
    assert dump(bcf, 1, 3) == bm.dump_text(rows)                        # the same rows, and the status of the shared rule
    assert all(st == bm.BCFIN_OK for _, st, _, _ in rows)               # no record of a golden input is handed back


@pytest.mark.parametrize("path", tvc.GOLDEN, ids=tvc.IDS)
def test_model_rows_equal_the_text_model_on_the_same_genotypes(path, golden_bcfs):
    """the device contract on the BCF = the device contract of the text parser on the VCF it was made from"""
    source = tvc._source(path)
    text_rows = tvc._device_rows(path, source)                          # [(pos, row, allelesum, status)]
    raw = bm.read_raw(golden_bcfs[(path, "u")])
    samples, recs = bm.parse_bcf(raw)
    assert len(recs) == len(text_rows)
    for r, (pos, row, total, st) in zip(recs, text_rows):
        ra = bm.allele_map_of(r["alleles"], 1)
        got = bm.plain_record(raw, r["gt_begin"], r["gt_type"], r["gt_n"], len(r["alleles"]), ra, len(samples))
        assert got[2] == bm.BCFIN_OK == st and r["pos"] == pos and got[1] == total and np.array_equal(got[0], row)


def write_odd_bcf(tmp_path):
    data, fallback = bc.odd_bcf()
    path = str(tmp_path / "odd.bcf")
    open(path, "wb").write(data)
    return path, fallback


def test_hook_equals_the_model_on_the_odd_records(tmp_path):
    path, fallback = write_odd_bcf(tmp_path)
    rows = bm.file_rows(open(path, "rb").read(), 1)
    assert {pos for pos, st, _, _ in rows if st == bm.BCFIN_HOST} == fallback and 0 < len(fallback) < len(rows) == len(bc.ODD_RECORDS)
    assert dump(path, 1, 3) == bm.dump_text(rows) and dump(path, 1, 0) == bm.dump_text(rows, status=-1)
    by_pos = {pos: (total, bytes(row).hex()) for pos, st, total, row in rows}
    # G,T,A,C,<*> -> 2,3,0,1,4: 0|1, 1/1, ./., .|1, 4|3; haploid 0 1 . 4 and nothing at all; the value 514 of int16 is allele 0 on the host
    assert by_pos[2] == (11, "32" "33" "ff" "3f" "14") and by_pos[7] == (10, "22" "33" "ff" "44" "ff") and by_pos[12][1][4:6] == "02"
    assert by_pos[5] == by_pos[6] and by_pos[13][1].startswith("ffff")  # int16 = int32; v0 = E with anything behind it


# ---- the boundary of the plain rule ---------------------------------------------------------------------------------------------
E, M = bm.END, bm.MISSING


@pytest.mark.parametrize("vals,nal,want", [
    ([2, 5], 2, (0, 1)), ([0, 1], 1, (-1, -1)), ([0, 4], 2, (-1, 1)), ([4], 2, (1, 1)), ([4, E], 2, (1, 1)), ([E], 2, (-1, -1)),
    ([E, E], 2, (-1, -1)), ([E, M], 2, (-1, -1)), ([E, -3], 2, (-1, -1)), ([E, 100], 2, (-1, -1)), ([10, 11], 5, (4, 4)),
    ([2, 4, M], 2, (0, 1)), ([2, 4, -9, 200], 2, (0, 1)), ([2, E, M], 2, (0, 0)),
    ([M], 2, None), ([M, 2], 2, None), ([2, M], 2, None), ([-1, 2], 2, None), ([2, -1], 2, None), ([-126, 2], 2, None),
    ([6, 2], 2, None), ([2, 7], 2, None), ([12, 2], 5, None), ([2, 13], 5, None), ([514, 2], 5, None), ([127], 5, None),
])
def test_plain_samples(vals, nal, want):
    assert bm.plain_sample(vals, nal) == want
    if want is not None:
        assert bm.host_sample(vals) == want                           # inside the rule the host's loop gives the same alleles


def test_typed_values():
    assert [bm.value(b"\x80\x81\x82\x7f\xff", i, 1) for i in range(5)] == [M, E, -126, 127, -1]
    assert [bm.value(b"\x00\x80\x01\x80\x81\xff\x02\x02", i, 2) for i in (0, 2, 4, 6)] == [M, E, -127, 514]
    assert [bm.value(b"\x00\x00\x00\x80\x01\x00\x00\x80\x81\x00\x00\x00", i, 4) for i in (0, 4, 8)] == [M, E, 129]
    for w in (1, 2, 4):
        assert bm.value(bm.encode("E", w), 0, w) == E and bm.value(bm.encode("M", w), 0, w) == M and bm.value(bm.encode(-3, w), 0, w) == -3


def test_host_rules_on_records_outside_the_rule():
    """what the host program computes for the values the device hands back ((int8_t) of the allele index, make_site's range check)"""
    assert bm.host_sample([M, 4]) == (-1, 1) and bm.host_sample([4, M]) == (1, -1) and bm.host_sample([-3, 2]) == (-3, 0)
    assert bm.host_sample([514, 2]) == (0, 0) and bm.host_sample([512, 2]) == (-1, 0) and bm.host_sample([2, 4, 6]) == (0, 1)
    with pytest.raises(bm.ModelDie):
        bm.host_record(bytes([2, 6]), 0, 1, 2, 2, bc.MAP_BINARY, 1)     # allele index 2 of two alleles
    with pytest.raises(bm.ModelDie):
        bm.host_record(bytes(8), 0, 5, 2, 2, bc.MAP_BINARY, 1)          # a float vector


def test_every_fallback_kind_is_handed_back_and_every_plain_edge_is_not():
    c = bc.case_fallback()
    rows, sums, status = c.expected()
    assert len(c.fallback) == len(bc.FALLBACK_KINDS) >= 20 and len(status) == 2 * len(bc.FALLBACK_KINDS) + 1
    for i in range(len(status)):
        assert status[i] == (bm.BCFIN_HOST if i in c.fallback else bm.BCFIN_OK), i
    e = bc.case_plain_edges()
    assert not e.expected()[2].any() and len(e.begin) == len(bc.PLAIN_EDGES) >= 8


@pytest.mark.parametrize("name", sorted(bc.all_cases()))
def test_fallback_share_of_the_kernel_inputs(name):
    """exactly the records constructed to be handed back are (none at all outside the fallback case)"""
    c = bc.all_cases()[name]
    rows, sums, status = c.expected()
    assert {int(i) for i in np.nonzero(status)[0]} == c.fallback
    assert bool(c.fallback) == (name == "fallback")
    assert sums.max() > 0 or c.N < 3


def test_the_bcf_writer_of_the_tests_reads_back(tmp_path):
    """tests/bcfin_cases.py binary_bcf -> the host reader: the packed rows it was made from"""
    import synth
    gt = synth.binary_sites(0, 9, 13)
    path = str(tmp_path / "b.bcf")
    open(path, "wb").write(bc.binary_bcf(gt))
    lines = dump(path, 1, 3).splitlines()
    assert [l.split()[3] for l in lines] == [bytes(r).hex() for r in gt] and all(l.split()[1] == "0" for l in lines)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
NEW = ["vgl_bcfin_workspace_bytes", "vgl_bcfin_decode_device", "vgl_bcfin_host_create", "vgl_bcfin_host_submit", "vgl_bcfin_host_wait",
       "vgl_bcfin_host_destroy"]


def test_declarations():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define\s+VGL_ABI_VERSION\s+7\b", hdr) and _abi.ABI_VERSION == 7
    assert re.search(r"#define\s+VGL_BCFIN_OK\s+0\b", hdr) and re.search(r"#define\s+VGL_BCFIN_HOST\s+1\b", hdr)
    assert (_abi.BCFIN_OK, _abi.BCFIN_HOST) == (bm.BCFIN_OK, bm.BCFIN_HOST) == (0, 1)
    lib = _abi.load_library()
    for name in NEW:
        assert re.search(r"VGL_API\s+\w+\s+%s\(" % name, hdr), name
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes, name
    assert ("header's %d entry points" % len(_abi.EXPORTS)) in open(os.path.join(ROOT, "README.md")).read()     # the README counts them
    assert lib.vgl_abi_version() == 7
    assert lib.vgl_bcfin_workspace_bytes(1000, 4096) > 0 and lib.vgl_bcfin_workspace_bytes(0, 1) == -1 and lib.vgl_bcfin_workspace_bytes(1, -1) == -1
    from vcfgl_amd import bcfin
    assert callable(bcfin.decode_gt) and (bcfin.BCFIN_OK, bcfin.BCFIN_HOST) == (0, 1)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_bcfin_host_create(0, 0, 16, 1024, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_host_create(0, 8, 0, 1024, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_host_create(0, 8, 16, 0, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_host_create(0, 8, 16, 1024, None) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_host_destroy(None) == _abi.VGL_OK
    assert lib.vgl_bcfin_host_submit(None, None, 0, 0, None, None, None, None, None, None) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_host_wait(None, 0, None, None, None) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_decode_device(0, None, 10, 1, None, None, None, None, None, 4, None, None, None, None, None) == _abi.VGL_E_ARG
    assert lib.vgl_bcfin_decode_device(0, None, -1, 0, None, None, None, None, None, 4, None, None, None, None, None) == _abi.VGL_E_ARG


@pytest.mark.skipif(tvc._have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_entry_points_are_refused():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_bcfin_host_create(0, 8, 16, 1024, C.byref(h)) == _abi.VGL_E_NODEVICE
    assert not h.value and b"vgl_bcfin_host_create" in lib.vgl_last_error()
    buf = (C.c_uint8 * 256)()                                          # (never touched: the device count is asked first)
    p = C.addressof(buf)
    assert lib.vgl_bcfin_decode_device(0, p, 16, 1, p, p, p, p, p, 4, p, p, p, p, None) == _abi.VGL_E_NODEVICE
    assert b"vgl_bcfin_decode_device" in lib.vgl_last_error()


# ---- the flag ---------------------------------------------------------------------------------------------------------------------
def test_help_names_the_flag():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--device-bcf-input 0|1" in r.stdout + r.stderr


def test_the_flag_is_refused_with_depth_inf_with_text_input_and_out_of_range(tmp_path, golden_bcfs):
    """each before any file of the run exists, the .arg file included"""
    bcf = golden_bcfs[(os.path.join(DATA, "data2.vcf"), "u")]
    out = str(tmp_path / "o")
    base = ["-o", out, "--seed", "1", "-e", "0.01", "--source", "1", "-O", "v"]
    r = run(["-i", bcf, "--depth", "inf", "--device-bcf-input", "1"] + base, ok=False)
    assert r.returncode != 0 and "--device-bcf-input 1 is not supported with --depth inf" in r.stderr and os.listdir(str(tmp_path)) == []
    r = run(["-i", bcf, "--depth", "1", "--device-bcf-input", "2"] + base, ok=False)
    assert r.returncode != 0 and "--device-bcf-input" in r.stderr and os.listdir(str(tmp_path)) == []
    for text in (os.path.join(DATA, "data2.vcf"),):
        r = run(["-i", text, "--depth", "1", "--device-bcf-input", "1"] + base, ok=False)
        assert r.returncode != 0 and "--device-bcf-input 1 needs BCF input" in r.stderr and os.listdir(str(tmp_path)) == []
    # --device-input 1 with a BCF stays refused, with its message
    r = run(["-i", bcf, "--depth", "1", "--device-input", "1", "--device-bcf-input", "1"] + base, ok=False)
    assert r.returncode != 0 and "--device-input 1 is not supported with BCF input (its genotypes are binary already: there is no text to parse)." in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_flag_off_reads_a_bcf_as_before(tmp_path, golden_bcfs):
    """--device-bcf-input 0 is the default: the same files with and without it, no GPU needed with --depth inf"""
    bcf = golden_bcfs[(os.path.join(DATA, "data5_acgt_multiallelic.vcf"), "b")]
    argv = ["--seed", "1", "--depth", "inf", "-e", "0", "--source", "1", "-O", "v", "-printTruth", "1"]
    run(["-i", bcf, "-o", str(tmp_path / "a")] + argv)
    run(["-i", bcf, "-o", str(tmp_path / "b"), "--device-bcf-input", "0"] + argv)
    def body(f):
        return [l for l in open(str(tmp_path / f)) if not l.startswith("##")]          # (the header records the command line)
    for ext in (".vcf", ".truth.vcf"):
        assert body("a" + ext) == body("b" + ext) and len(body("a" + ext)) > 3


@pytest.mark.skipif(tvc._have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_program_fails_instead_of_falling_back(tmp_path, golden_bcfs):
    bcf = golden_bcfs[(os.path.join(DATA, "data2.vcf"), "u")]
    r = run(["-i", bcf, "-o", str(tmp_path / "o"), "--seed", "1", "--depth", "1", "-e", "0.01", "--source", "1", "-O", "v", "--device-bcf-input", "1"], ok=False)
    assert r.returncode != 0 and "--device-bcf-input 1:" in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith((".vcf", ".bcf", ".gz"))]
    r = run(["--dump-gt", bcf, "1", "2"], ok=False)
    assert r.returncode != 0 and "--device-bcf-input 1:" in r.stderr
