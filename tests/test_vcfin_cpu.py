"""The input parser without a GPU: tests/vcfin_model.py (the statement of what the device parser computes) against the Python record
loop and against the host program's own parser (vcfgl_hip --dump-gt FILE SOURCE 0), the boundary of the plain grammar, the
fallback share of every synthetic input of the GPU tests, the declarations, and the refusals of a machine without a device."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import vcfin_cases as vc
import vcfin_model as vm
from vcfgl_amd import _abi
from vcfgl_amd import recordloop, vcfio
from vcfgl_amd.params import VcfglArgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")


def _is_input(path):
    """a golden .vcf that is an input the program accepts: its records carry GT (the others are expected outputs) and as many sample
    columns as the header names (data8.vcf has one more: the program exits on it, see test_a_line_with_another_column_count)"""
    text, samples, lines = vm.read_lines(path)
    cols = [text[a:b].split(b"\t") for a, b in lines]
    return bool(lines) and all(len(c) == 9 + len(samples) and b"GT" in c[8].split(b":") for c in cols)


def _source(path):
    text, samples, lines = vm.read_lines(path)
    return 1 if all(text[a:b].split(b"\t")[3] in (b"A", b"C", b"G", b"T") for a, b in lines) else 0


GOLDEN = sorted(p for p in glob.glob(os.path.join(gu.REFVCF, "data", "*.vcf")) + glob.glob(os.path.join(gu.GOLD, "doc_msprime", "*.vcf"))
                if _is_input(p))
IDS = [os.path.basename(p) for p in GOLDEN]


def test_the_golden_inputs_are_found():
    assert sorted(IDS) == sorted(["data1.vcf", "data2.vcf", "data3.vcf", "data4_acgt_biallelic.vcf", "data4_acgt_biallelic_a2g_c2t.vcf",
                          "data4_binary_biallelic.vcf", "data5_acgt_multiallelic.vcf", "data6.vcf", "data7.vcf", "msprime_output.vcf"])
    every = glob.glob(os.path.join(gu.REFVCF, "data", "*.vcf")) + glob.glob(os.path.join(gu.GOLD, "doc_msprime", "*.vcf"))
    # the others: two expected gVCF outputs and one expected output (no GT), and data8.vcf (a column more than its header names)
    assert sorted(os.path.basename(p) for p in every if p not in GOLDEN) == ["data1_g1_gvcf.vcf", "data1_g2_gvcf.vcf", "data8.vcf", "sim_source0.vcf"]
    assert {_source(p) for p in GOLDEN} == {0, 1}


def _device_rows(path, source):
    """the model's device contract over a file: [(pos, row, allelesum, status)]"""
    text, samples, lines = vm.read_lines(path)
    out = []
    for ls, le in lines:
        f = vm.fixed(text, ls, le, source)
        assert f["describable"]
        row, total, st = vm.plain_line(text, f["line_begin"], le, f["gti"], f["n_alleles"], f["allele_map"], len(samples))
        out.append((f["pos"], row, total, st))
    return out


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_model_equals_the_python_record_loop(path):
    """an independent route to the same rows: vcfio.read_vcf + recordloop.check_rec_alleles"""
    source = _source(path)
    vcf = vcfio.read_vcf(path)
    args = VcfglArgs(source=source)
    ours = _device_rows(path, source)
    assert len(ours) == len(vcf.records) > 0
    for (pos, row, total, st), rec in zip(ours, vcf.records):
        status, want = recordloop.check_rec_alleles(rec, args, len(vcf.samples))
        assert st == vm.VCFIN_OK and status == 0 and pos == rec.pos0 + 1
        assert np.array_equal(row, want)
        assert total == sum(max(a, 0) + max(b, 0) for a, b in rec.gts)


def test_no_golden_line_falls_back():
    n = fb = 0
    for path in GOLDEN:
        for _, _, _, st in _device_rows(path, _source(path)):
            n += 1
            fb += st != vm.VCFIN_OK
    assert n > 50 and fb == 0


def dump(path, source, device_input=0):
    r = subprocess.run([BIN, "--dump-gt", path, str(source), str(device_input)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_hook_equals_the_model_on_the_golden_inputs(path):
    source = _source(path)
    assert dump(path, source) == vm.dump_text(vm.file_rows(path, source))


def test_a_line_with_another_column_count():
    """data8.vcf: ten sample columns under a header of nine names.  The model hands every such line to the host, whose parser exits"""
    path = os.path.join(gu.REFVCF, "data", "data8.vcf")
    text, samples, lines = vm.read_lines(path)
    assert len(samples) == 9 and path not in GOLDEN
    for ls, le in lines:
        f = vm.fixed(text, ls, le, 1)
        assert f["describable"]
        assert vm.plain_line(text, f["line_begin"], le, f["gti"], f["n_alleles"], f["allele_map"], 9)[2] == vm.VCFIN_HOST
        assert vm.plain_line(text, f["line_begin"], le, f["gti"], f["n_alleles"], f["allele_map"], 10)[2] == vm.VCFIN_OK
    r = subprocess.run([BIN, "--dump-gt", path, "1", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "has 10 sample columns, the header names 9 samples" in r.stderr


def write_odd_lines(tmp_path):
    data, fallback = vc.odd_lines_vcf()
    path = str(tmp_path / "odd.vcf")
    open(path, "wb").write(data)
    return path, fallback


def test_hook_equals_the_model_on_the_odd_lines(tmp_path):
    path, fallback = write_odd_lines(tmp_path)
    assert not open(path, "rb").read().endswith(b"\n")                 # a last line without a newline
    rows = vm.file_rows(path, 1)
    assert {pos for pos, st, _, _ in rows if st == vm.VCFIN_HOST} == fallback and 0 < len(fallback) < len(rows)
    assert dump(path, 1) == vm.dump_text(rows)
    by_pos = {pos: (total, bytes(row).hex()) for pos, st, total, row in rows}
    # G,T,A,C,<*> -> 2,3,0,1,4: ".", "./.", ".|1", haploid "0", "1/0"; then "3|4"
    assert by_pos[2] == (2, "ff" "ff" "3f" "22" "23") and by_pos[3][1].startswith("41")
    assert by_pos[5][1] == "32" "33" "ff" "10" "42" and by_pos[6][1] == "32" "33" "ff" "10" "44"      # 0|1:35:1,2 and 35:0|1 -> 0|1
    assert by_pos[7] == (3, "32" "ff" "ff" "33" "ff")                    # columns that end before GT have no token


# ---- the boundary of the plain grammar ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tok,want", [
    (b".", (-1, -1)), (b"./.", (-1, -1)), (b".|1", (-1, 1)), (b"0", (0, 0)), (b"1/0", (1, 0)), (b"3|4", (3, 4)), (b"01|04", (1, 4)), (b"00", (0, 0)),
    (b"", None), (b"0|", None), (b"|0", None), (b"0|1|0", None), (b"0/1/0", None), (b"001", None), (b"0|001", None), (b".1", None), (b"..", None),
    (b"0|5", None), (b"5", None), (b"10|0", None), (b"0|1\r", None), (b"0 |1", None), (b"-1", None), (b"+1", None), (b"0\\1", None), (b"a", None),
])
def test_plain_tokens(tok, want):
    assert vm.plain_token(tok, 5) == want
    if want is not None:
        assert vm.host_token(tok) == want                             # inside the grammar the host's rule gives the same alleles


def test_every_fallback_kind_is_sent_to_the_host():
    c = vc.case_fallback()
    rows, sums, status = c.expected()
    assert len(c.fallback) == len(vc.FALLBACK_KINDS) >= 10
    for i in range(len(status)):
        assert status[i] == (vm.VCFIN_HOST if i in c.fallback else vm.VCFIN_OK), i


@pytest.mark.parametrize("name", sorted(vc.all_cases()))
def test_fallback_share_of_the_kernel_inputs(name):
    """exactly the lines constructed to fall back do (none at all outside the fallback case)"""
    c = vc.all_cases()[name]
    rows, sums, status = c.expected()
    assert {int(i) for i in np.nonzero(status)[0]} == c.fallback
    assert bool(c.fallback) == (name == "fallback")


def test_host_rules_on_lines_outside_the_grammar():
    """what the host program computes for the tokens the device hands back (atoi on the allele bytes, int8, a1 = a0)"""
    assert vm.host_token(b"0|1|1") == (0, 1) and vm.host_token(b"0|") == (0, -1) and vm.host_token(b"001") == (1, 1)
    assert vm.host_token(b"0|1\r") == (0, 1) and vm.host_token(b".1") == (-1, -1) and vm.host_token(b"") == (-1, -1)
    assert vm.host_token(b"200") == (-56, -56) and vm.host_token(b"0|x") == (0, 0)
    with pytest.raises(vm.ModelDie):
        vm.host_line(b"0|2\t0|0", 0, 7, 0, 2, vc.MAP_BINARY, 2)
    with pytest.raises(vm.ModelDie):
        vm.host_line(b"0|0\t0|0\t0|0", 0, 11, 0, 2, vc.MAP_BINARY, 2)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
NEW = ["vgl_vcfin_workspace_bytes", "vgl_vcfin_parse_device", "vgl_vcfin_host_create", "vgl_vcfin_host_submit", "vgl_vcfin_host_wait",
       "vgl_vcfin_host_destroy"]


def test_declarations():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define\s+VGL_ABI_VERSION\s+7\b", hdr) and _abi.ABI_VERSION == 7
    assert re.search(r"#define\s+VGL_VCFIN_OK\s+0\b", hdr) and re.search(r"#define\s+VGL_VCFIN_HOST\s+1\b", hdr)
    assert (_abi.VCFIN_OK, _abi.VCFIN_HOST) == (vm.VCFIN_OK, vm.VCFIN_HOST) == (0, 1)
    lib = _abi.load_library()
    for name in NEW:
        assert re.search(r"VGL_API\s+\w+\s+%s\(" % name, hdr), name
        assert name in _abi.EXPORTS and getattr(lib, name).argtypes, name
    assert lib.vgl_abi_version() == 7
    assert lib.vgl_vcfin_workspace_bytes(1000, 4096) > 0 and lib.vgl_vcfin_workspace_bytes(0, 1) == -1
    from vcfgl_amd import vcfin
    assert callable(vcfin.parse_gt)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_vcfin_host_create(0, 0, 16, 1024, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_vcfin_host_create(0, 8, 0, 1024, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_vcfin_host_create(0, 8, 16, 0, C.byref(h)) == _abi.VGL_E_ARG
    assert lib.vgl_vcfin_host_create(0, 8, 16, 1024, None) == _abi.VGL_E_ARG
    assert lib.vgl_vcfin_host_destroy(None) == _abi.VGL_OK
    assert lib.vgl_vcfin_parse_device(0, None, 10, 1, None, None, None, None, None, 4, None, None, None, None, None) == _abi.VGL_E_ARG
    assert lib.vgl_vcfin_parse_device(0, None, -1, 0, None, None, None, None, None, 4, None, None, None, None, None) == _abi.VGL_E_ARG


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_entry_points_are_refused():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_vcfin_host_create(0, 8, 16, 1024, C.byref(h)) == _abi.VGL_E_NODEVICE
    assert not h.value and b"vgl_vcfin_host_create" in lib.vgl_last_error()
    buf = (C.c_uint8 * 256)()                                          # (never touched: the device count is asked first)
    p = C.addressof(buf)
    assert lib.vgl_vcfin_parse_device(0, p, 16, 1, p, p, p, p, p, 4, p, p, p, p, None) == _abi.VGL_E_NODEVICE
    assert b"vgl_vcfin_parse_device" in lib.vgl_last_error()


def test_depth_inf_is_refused_and_nothing_is_written(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN, "-i", os.path.join(gu.REFVCF, "data", "data2.vcf"), "-o", out, "--seed", "1", "--depth", "inf", "-e", "0", "-O", "v",
                        "--device-input", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-input 1 is not supported with --depth inf" in r.stderr
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([BIN, "-i", os.path.join(gu.REFVCF, "data", "data2.vcf"), "-o", out, "--seed", "1", "--depth", "1", "-e", "0", "-O", "v",
                        "--device-input", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-input" in r.stderr and os.listdir(str(tmp_path)) == []


@pytest.mark.skipif(_have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_without_a_device_the_program_fails_instead_of_falling_back(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN, "-i", os.path.join(gu.REFVCF, "data", "data2.vcf"), "-o", out, "--seed", "1", "--depth", "1", "-e", "0.01", "-O", "v",
                        "--device-input", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-input 1:" in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith((".vcf", ".bcf", ".gz"))]
