"""The set-alleles additions of the C ABI without a device: the symbols exist (library, header, _abi.EXPORTS), the workspace size is
the documented arithmetic, and the argument checks that precede any device call return VGL_E_ARG."""
import os
import re

from vcfgl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vgl_setal_workspace_bytes", "vgl_setal_apply_device", "vgl_ctx_set_alleles"]


def test_symbols_in_the_library_the_header_and_the_export_list():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.EXPORTS
        assert re.search(r"VGL_API\s+\w+\s+%s\(" % name, header), name
    assert re.search(r"#define VGL_E_SETAL\s+\(-8\)", header) and _abi.VGL_E_SETAL == -8
    assert lib.vgl_abi_version() == _abi.ABI_VERSION == 7       # additive: the version stays


def test_workspace_arithmetic():
    lib = _abi.load_library()
    ws = lib.vgl_setal_workspace_bytes
    plan = lambda s: (32 * s + 255) // 256 * 256                 # one 32-byte plan per site, rounded up to 256 bytes
    for n, s, g in [(1, 1, 10), (65, 37, 15), (257, 4096, 15), (32768, 4096, 15), (0, 0, 0), (5, 0, 15)]:
        assert ws(n, s, g) == plan(s) + 4 * n * s * g, (n, s, g)
    assert ws(-1, 1, 10) == ws(1, -1, 10) == ws(1, 1, -1) == -1
    assert ws(2 ** 31 - 1, 2 ** 31 - 1, 15) == -1                # does not fit 63 bits


def test_bad_arguments_return_e_arg_before_any_device_call():
    lib = _abi.load_library()
    p = 4096                                                     # never dereferenced: every case fails its check first
    ok = [0, 1, 1, 10, 4, _abi.VGL_LAYOUT_PLANES, p, p, p, p, None, None, None, None, None, None, p, p, 1 << 20, None]
    cases = [(1, 0), (1, -3), (2, -1), (3, 0), (3, 16), (4, 0), (4, 6), (5, 2), (5, -1), (6, None), (7, None), (8, None), (9, None),
             (16, None), (17, None), (18, 8), (18, -1)]
    for k, v in cases:
        a = list(ok)
        a[k] = v
        assert lib.vgl_setal_apply_device(*a) == _abi.VGL_E_ARG, (k, v)
        assert b"vgl_setal_apply_device" in lib.vgl_last_error()
    a = list(ok)
    a[15] = p                                                    # pl_u8 without fmt_dp
    assert lib.vgl_setal_apply_device(*a) == _abi.VGL_E_ARG and b"fmt_dp" in lib.vgl_last_error()
    a = list(ok)
    a[2] = 0                                                     # no sites: nothing to do, nothing is looked at
    a[6:10] = [None] * 4
    assert lib.vgl_setal_apply_device(*a) == _abi.VGL_OK
    assert lib.vgl_ctx_set_alleles(None, None, 0, 0) == _abi.VGL_E_ARG
