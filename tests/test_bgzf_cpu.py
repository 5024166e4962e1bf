"""The device BGZF compressor's host surface without a GPU: the --device-bgzf flag of the host program, the ABI 7 entry points in
include/vcfgl_hip.h and the ctypes mirror, and vgl_bgzf_bound / vgl_bgzf_workspace_bytes (pure host arithmetic)."""
import os
import re
import subprocess

import pytest

from vcfgl_amd import _abi, bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
NEW = ("vgl_bgzf_bound", "vgl_bgzf_workspace_bytes", "vgl_bgzf_compress_device")


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_help_lists_device_bgzf():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--device-bgzf 0|1" in r.stderr


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_device_bgzf_2_is_refused(tmp_path):
    vcf = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data", "data3.vcf")
    r = subprocess.run([BIN, "-i", vcf, "-o", str(tmp_path / "o"), "--depth", "inf", "-e", "0", "--seed", "1", "--device-bgzf", "2"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--device-bgzf" in r.stderr and "Allowed range is [0,1]" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.bcf"))


def test_header_and_exports_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    for name in NEW:
        assert re.search(r"VGL_API\s+\w+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    assert "#define VGL_ABI_VERSION 7" in hdr and _abi.ABI_VERSION == 7


def test_bound_covers_the_stored_form():
    lib = _abi.load_library()
    M = bgzf.MEMBER_BYTES
    for n in (0, 1, 2, 100, M - 1, M, M + 1, 2 * M, 3 * M + 17, 1000 * M + 5, 10 ** 9, 2 ** 33 + 7):
        members = -(-n // M)
        stored = sum(18 + 5 + min(M, n - k * M) + 8 for k in range(members)) if members < 5000 else n + 31 * members
        b = lib.vgl_bgzf_bound(n)
        assert b >= stored and b == bgzf.bound(n), (n, b, stored)
        assert lib.vgl_bgzf_workspace_bytes(n) >= (0 if n == 0 else n)
    assert lib.vgl_bgzf_bound(-1) == -1 and lib.vgl_bgzf_workspace_bytes(-1) == -1
    assert bgzf.EOF == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_compress_device_rejects_a_short_destination():
    lib = _abi.load_library()
    # checked before any device is touched
    rc = lib.vgl_bgzf_compress_device(0, 1, 100, 1, 100, None, 1, 1 << 30, None)
    assert rc == _abi.VGL_E_ARG and b"vgl_bgzf_bound" in lib.vgl_last_error()
