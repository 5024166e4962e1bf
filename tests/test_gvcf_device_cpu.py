"""No-GPU checks of the device gVCF blocker's surroundings: the C ABI declarations of the new entry points, the ctypes structures
against the header's, and the host program's refusals of --device-gvcf."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import golden_util as gu
from vcfgl_amd import _abi, gvcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
ENTRIES = ["vgl_gvcf_workspace_bytes", "vgl_gvcf_blocks_device", "vgl_ctx_gvcf_text_bound", "vgl_simulate_tile_gvcf_async"]
STRUCTS = {"vgl_gvcf_item": _abi.GvcfItem, "vgl_gvcf_in": _abi.GvcfIn, "vgl_gvcf_out": _abi.GvcfOut, "vgl_gvcf_tile": _abi.GvcfTile}


def test_header_declares_the_gvcf_entries():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define VGL_ABI_VERSION 7\b", hdr) and _abi.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(r"VGL_API\s+\w+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    for name, v in (("VGL_GVCF_RECORD", 0), ("VGL_GVCF_BLOCK", 1)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), hdr), name
    lib = _abi.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert lib.vgl_gvcf_workspace_bytes(3, 10) > 0 and lib.vgl_gvcf_workspace_bytes(-1, 10) == -1


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every member offset of the four structures, compiled from the header, against the ctypes mirrors"""
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    assert cc, "no C compiler"
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "vcfgl_hip.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append("return 0; }")
    c_file, exe = tmp_path / "layout.c", tmp_path / "layout"
    c_file.write_text("\n".join(src) + "\n")
    lang = ["-x", "c"] if not cc.endswith("hipcc") else ["-x", "c++"]
    subprocess.run([cc] + lang + [str(c_file), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, py in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_exist():
    assert callable(gvcf.blocks_device) and callable(gvcf.blocks_device_raw) and issubclass(gvcf.GvcfError, ValueError)


GV = ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1", "-doUnobserved", "2"]
# (argv, what the message says besides the flag)
REFUSED = {
    "bad value": (["-O", "v", "--device-gvcf", "2"] + GV, "Allowed range is [0,1]"),
    "no gvcf": (["-O", "v", "--device-gvcf", "1"], "-doGVCF 1"),
    "bcf": (["-O", "b", "--device-gvcf", "1"] + GV, "-O v or -O z"),
    "ubcf": (["-O", "u", "--device-gvcf", "1"] + GV, "-O v or -O z"),
    "depth inf": (["-O", "v", "--device-gvcf", "1", "--depth", "inf"] + GV, "--depth inf"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refuses_device_gvcf_where_it_cannot_apply(case, tmp_path):
    assert os.path.exists(BIN), "vcfgl_hip not built"
    out = str(tmp_path / "o")
    flags, why = REFUSED[case]
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "--seed", "1", "-e", "0.01"] + flags
    if "--depth" not in argv:
        argv += ["--depth", "2"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert "--device-gvcf" in r.stderr and why in r.stderr and "Unknown argument" not in r.stderr
    assert not os.listdir(str(tmp_path))                       # refused before anything is written


def test_device_text_with_gvcf_points_to_device_gvcf(tmp_path):
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", str(tmp_path / "o"), "--seed", "1", "-e", "0.01", "--depth", "2", "-O", "v",
            "--device-text", "1"] + GV
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--device-text" in r.stderr and "-doGVCF 1" in r.stderr and "--device-gvcf 1" in r.stderr
    assert not os.listdir(str(tmp_path))


def test_usage_lists_the_flag():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert "--device-gvcf 0|1" in r.stdout + r.stderr
