"""No-GPU checks of the device VCF text formatter's surroundings: the Python model of the text (tests/vcftext_model.py) against the host
program's own float formatter, the C ABI declarations of the new entry points, and the host program's refusals of --device-text."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import vcftext_model as vm
from vcfgl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
ENTRIES = ["vgl_text_bound", "vgl_text_workspace_bytes", "vgl_text_format_device", "vgl_ctx_text_bound", "vgl_simulate_tile_text_async"]


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_model_formats_floats_as_the_host_program():
    """every class boundary of put_float (+-0, denormals, FLT_MIN, 1e-4 and 999999 +- ulps, decade roll-overs, integer-valued ties above
    1e6, +-inf, NaN payloads, the missing pattern) and random patterns: the model and `vcfgl_hip --format-floats` agree token for token"""
    pats = vm.float_corpus()
    assert len(pats) > 90000
    got = []
    for i in range(0, len(pats), 4000):
        r = subprocess.run([BIN, "--format-floats"] + ["%08x" % p for p in pats[i:i + 4000]], capture_output=True, text=True, check=True)
        got += r.stdout.split("\n")[:-1]
    assert len(got) == len(pats)
    bad = [(hex(p), g, vm.fmt_float_bits(p)) for p, g in zip(pats, got) if g != vm.fmt_float_bits(p)]
    assert not bad, bad[:20]


def test_model_ints_and_layout():
    assert [vm.fmt_int(v) for v in (vm.INT32_MISSING, vm.INT32_MISSING + 1, -7, 0, 2 ** 31 - 1)] == [".", "-2147483647", "-7", "0", "2147483647"]
    # two sites (the second skipped), two samples: DP (one value), GL (nG = 3 at nA = 2) and AD (nA), sample-major slabs
    dp = np.array([[3, 4], [0, 0]], dtype=np.int32)
    gl = np.zeros((2, 2 * 15), dtype=np.float32)
    gl[0, :6] = [0, -0.5, -1.25, -2, 0, -1e-5]
    ad = np.zeros((2, 2 * 5), dtype=np.int32)
    ad[0, :4] = [1, 2, 3, vm.INT32_MISSING]
    text, off = vm.render([("DP", dp, vm.ONE), ("GL", gl, vm.PER_G), ("AD", ad, vm.PER_A)], np.array([0, -3]), np.array([2, 2]), 2)
    assert text == b"\tDP:GL:AD\t3:0,-0.5,-1.25:1,2\t4:-2,0,-1e-05:3,.\n"
    assert list(off) == [0, len(text), len(text)]
    assert vm.render([], np.array([0]), np.array([1]), 3)[0] == b"\t.\t.\t.\t.\n"


def test_header_declares_the_text_entries():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define VGL_ABI_VERSION 7\b", hdr) and _abi.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(r"VGL_API\s+\w+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    for name, v in (("VGL_TEXT_ONE", 0), ("VGL_TEXT_PER_G", 1), ("VGL_TEXT_PER_A", 2), ("VGL_TEXT_MAX_FIELDS", 8)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), hdr), name
    import ctypes as C
    assert C.sizeof(_abi.TextField) == 32


def test_vcftext_is_a_submodule_only():
    import vcfgl_amd
    src = open(os.path.join(ROOT, "vcfgl_amd", "__init__.py")).read()
    assert "vcftext" not in src
    from vcfgl_amd import vcftext
    assert [k for k, *_ in vcftext.FORMAT_ORDER] == ["DP", "GL", "PL", "GP", "AD", "ADF", "ADR"]


# (argv, what the message says besides the flag)
REFUSED = {
    "bad value": (["-O", "v", "--device-text", "2"], "Allowed range is [0,1]"),
    "bcf": (["-O", "b", "--device-text", "1"], "-O v or -O z"),
    "ubcf": (["-O", "u", "--device-text", "1"], "-O v or -O z"),
    "gvcf": (["-O", "v", "--device-text", "1", "-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1"], "-doGVCF 1"),
    "depth inf": (["-O", "z", "--device-text", "1", "--depth", "inf"], "--depth inf"),
}


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refuses_device_text_where_it_cannot_apply(case, tmp_path):
    out = str(tmp_path / "o")
    flags, why = REFUSED[case]
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "--seed", "1", "-e", "0.01"] + flags
    if "--depth" not in argv:
        argv += ["--depth", "2"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert "--device-text" in r.stderr and why in r.stderr and "Unknown argument" not in r.stderr
    assert not os.listdir(str(tmp_path))                       # refused before anything is written
