"""No-GPU checks of the device record stream's surroundings: the numpy model of the assembly (tests/stream_model.py) against a plain
join, the C ABI declarations of the new entry points, the handle without a device, and the host program's refusals of --device-stream."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import stream_model as sm
from vcfgl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
ENTRIES = ["vgl_stream_assemble_device", "vgl_ctx_text_device", "vgl_stream_host_create", "vgl_stream_host_body", "vgl_stream_host_submit",
           "vgl_stream_host_wait", "vgl_stream_host_destroy"]


def test_header_declares_the_stream_entries():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define VGL_ABI_VERSION 7\b", hdr) and _abi.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(r"VGL_API\s+[\w*]+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    assert re.search(r"typedef struct vgl_stream_host vgl_stream_host;", hdr)
    assert len(set(_abi.EXPORTS)) == len(_abi.EXPORTS)


def test_the_library_exports_the_entries_with_argtypes():
    lib = _abi.load_library()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.vgl_stream_host_body.restype is C.c_void_p


def test_stream_is_a_submodule_only():
    import vcfgl_amd
    src = open(os.path.join(ROOT, "vcfgl_amd", "__init__.py")).read()
    assert "stream" not in src
    from vcfgl_amd import stream
    assert callable(stream.assemble) and callable(stream.assemble_into) and hasattr(stream.HostStream, "submit")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="needs a machine WITHOUT a GPU")
def test_create_without_a_device_is_refused():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.vgl_stream_host_create(0, 2, 64, 1 << 16, 1 << 20, C.byref(h)) == _abi.VGL_E_NODEVICE
    assert not h.value and b"vgl_stream_host_create" in lib.vgl_last_error()


def test_bad_create_arguments_are_refused_before_any_device_call():
    lib = _abi.load_library()
    h = C.c_void_p()
    for args, word in (((0, 0, 64, 10, 10), b"n_buffers"), ((0, 9, 64, 10, 10), b"n_buffers"), ((0, 2, 0, 10, 10), b"max_sites"),
                       ((0, 2, 64, 0, 10), b"max_head_bytes"), ((0, 2, 64, 10, 0), b"max_body_bytes")):
        assert lib.vgl_stream_host_create(*args, C.byref(h)) == _abi.VGL_E_ARG and word in lib.vgl_last_error(), word
    assert lib.vgl_stream_host_create(0, 2, 64, 10, 10, None) == _abi.VGL_E_ARG
    assert lib.vgl_stream_host_destroy(None) == _abi.VGL_OK
    assert lib.vgl_ctx_text_device(None, 1) == _abi.VGL_E_ARG


def lengths_to_offsets(lengths, base=0):
    return base + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_a_plain_join(seed):
    rng = np.random.default_rng(seed)
    n = [0, 1, 2, 17, 64, 300][seed]
    hl, bl = rng.integers(0, 40, n), rng.integers(0, 3000, n) * (rng.random(n) < 0.7)
    if n > 2:
        hl[1] = bl[1] = 0                                             # a site that contributes nothing
    hs = [bytes(rng.integers(0, 256, int(x), dtype=np.uint8)) for x in hl]
    bs = [bytes(rng.integers(0, 256, int(x), dtype=np.uint8)) for x in bl]
    heads, bodies = np.frombuffer(b"".join(hs), np.uint8), np.frombuffer(b"".join(bs), np.uint8)
    for bh, bb in ((0, 0), (11, 1 << 33)):                            # the offsets may start anywhere
        stream, rec = sm.assemble(heads, lengths_to_offsets(hl, bh), bodies, lengths_to_offsets(bl, bb))
        assert bytes(stream) == b"".join(h + b for h, b in zip(hs, bs))
        assert rec[0] == 0 and rec[-1] == len(stream) and np.array_equal(np.diff(rec), hl + bl)
        for i in range(n):
            assert bytes(stream[rec[i]:rec[i + 1]]) == hs[i] + bs[i]


GVCF = ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1", "-doUnobserved", "2"]
# (argv, the flag the message names, what it says besides)
REFUSED = {
    "bad value": (["-O", "b", "--device-bcf", "1", "--device-stream", "2"], "--device-stream", "Allowed range is [0,1]"),
    "negative value": (["-O", "z", "--device-text", "1", "--device-stream", "-1"], "--device-stream", "Allowed range is [0,1]"),
    "bcf": (["-O", "u", "--device-bcf", "1", "--device-stream", "1"], "--device-stream", "-O b or -O z"),
    "vcf": (["-O", "v", "--device-text", "1", "--device-stream", "1"], "--device-stream", "-O b or -O z"),
    "vcf alone": (["-O", "v", "--device-stream", "1"], "--device-stream", "-O b or -O z"),
    "b without bcf": (["-O", "b", "--device-stream", "1"], "--device-stream", "--device-bcf 1"),
    "b without bcf, bgzf": (["-O", "b", "--device-bgzf", "1", "--device-stream", "1"], "--device-stream", "--device-bcf 1"),
    "z without text": (["-O", "z", "--device-stream", "1"], "--device-stream", "--device-text 1"),
    "gvcf, b": (["-O", "b", "--device-bcf", "1", "--device-gvcf", "1", "--device-stream", "1"] + GVCF, "--device-stream", "-doGVCF 1"),
    "gvcf, z": (["-O", "z", "--device-gvcf", "1", "--device-stream", "1"] + GVCF, "--device-stream", "-doGVCF 1"),
    "depth inf, b": (["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--depth", "inf"], "--device-stream", "--depth inf"),
    "depth inf, z": (["-O", "z", "--device-text", "1", "--device-stream", "1", "--depth", "inf"], "--device-stream", "--depth inf"),
    # what was refused before stays refused, with its present message
    "device bcf, z": (["-O", "z", "--device-bcf", "1"], "--device-bcf", "-O u or -O b"),
    "device bcf, depth inf": (["-O", "b", "--device-bcf", "1", "--depth", "inf"], "--device-bcf", "--depth inf"),
    "device text, b": (["-O", "b", "--device-text", "1"], "--device-text", "-O v or -O z"),
    "device text, gvcf": (["-O", "z", "--device-text", "1"] + GVCF, "--device-text", "-doGVCF 1"),
    "device text, depth inf": (["-O", "z", "--device-text", "1", "--depth", "inf"], "--device-text", "--depth inf"),
    "device gvcf, b": (["-O", "b", "--device-gvcf", "1"] + GVCF, "--device-gvcf", "-O v or -O z"),
    "device bgzf value": (["-O", "b", "--device-bgzf", "2"], "--device-bgzf", "Allowed range is [0,1]"),
    "vcf threads": (["-O", "z", "--device-text", "1", "--device-stream", "1", "--threads", "2"], "--threads 1", "Multithreading is not supported for VCF output"),
}


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refuses_device_stream_where_it_cannot_apply(case, tmp_path):
    out = str(tmp_path / "o")
    flags, flag, why = REFUSED[case]
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "--seed", "1", "-e", "0.01"] + flags
    if "--depth" not in argv:
        argv += ["--depth", "2"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert flag in r.stderr and why in r.stderr and "Unknown argument" not in r.stderr
    assert not os.listdir(str(tmp_path))                       # refused before anything is written


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_help_describes_the_flag():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--device-stream 0|1" in text and "members restart at every tile" in text


@pytest.mark.skipif(_have_gpu() or not os.path.exists(BIN), reason="needs a machine WITHOUT a GPU and the built program")
def test_a_run_without_a_gpu_fails_and_does_not_fall_back(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "-O", "b", "--seed", "1", "-e", "0.01", "--depth", "2", "--device-bcf", "1",
                        "--device-stream", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no HIP device available" in r.stderr
    assert not os.path.exists(out + ".bcf") and "Simulation finished successfully" not in r.stderr
