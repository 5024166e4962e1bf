"""No-GPU checks of the device BCF encoder's surroundings: the numpy model of the FORMAT part of a record (tests/bcf_model.py) against
the independent reader (tests/bcf_reader.py) and, byte for byte, against the host program's own integer typing and narrowing
(`vcfgl_hip --encode-ints`); the C ABI declarations of the new entry points; and the host program's refusals of --device-bcf."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bcf_model as bm
import bcf_reader
import golden_util as gu
from vcfgl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
ENTRIES = ["vgl_bcf_bound", "vgl_bcf_workspace_bytes", "vgl_bcf_encode_device", "vgl_ctx_bcf_keys"]
M, E = bm.INT32_MISSING, bm.INT32_VEND


def write_bcf(path, N, keys, records):
    """a BCF file of records with a minimal shared block (contig c1, one allele per entry of `alleles`, no ID / FILTER / INFO) and the
    given FORMAT bytes; keys = [(id, name, type)]"""
    text = "##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"p\",IDX=0>\n##contig=<ID=c1,length=1000,IDX=0>\n"
    for idx, name, ty in keys:
        text += f"##FORMAT=<ID={name},Number=.,Type={ty},Description=\"x\",IDX={idx}>\n"
    text += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"s{i}" for i in range(N)) + "\n"
    raw = text.encode() + b"\0"
    out = b"BCF\2\2" + struct.pack("<I", len(raw)) + raw
    for pos0, alleles, n_fmt, indiv in records:
        shared = struct.pack("<iiiIII", 0, pos0, 1, bcf_reader.F_MISSING, len(alleles) << 16, n_fmt << 24 | N) + b"\x07"
        for a in alleles:
            shared += bytes([len(a) << 4 | 7]) + a.encode()
        shared += b"\x00"
        out += struct.pack("<II", len(shared), len(indiv)) + shared + indiv
    with open(path, "wb") as f:
        f.write(out)


def test_model_records_decode_through_the_independent_reader(tmp_path):
    """sites of 1, 2 and 5 alleles (15 values per sample), a skipped site, integers of every width with missing and vector-end values,
    floats with the missing pattern and a NaN payload: the reader gives the input values back"""
    N = 3
    rng = np.random.default_rng(5)
    na = np.array([2, 5, 1, 3, 5], dtype=np.int32)
    st = np.array([0, 0, 1, -3, 0], dtype=np.int32)
    S = len(na)
    dp = rng.integers(0, 100, (S, N)).astype(np.int32)
    pl = rng.integers(0, 100, (S, N * 15)).astype(np.int32)          # int8
    pl[0, 1], pl[0, 2] = M, E
    pl[1, :] = rng.integers(-300, 30000, N * 15)                     # int16, 15 values
    pl[1, 7] = M
    pl[4, :] = rng.integers(-70000, 70000, N * 15)                   # int32, 15 values
    pl[4, 0], pl[4, 44] = E, M
    gl = rng.standard_normal((S, N * 15)).astype(np.float32)
    glb = gl.view(np.uint32)
    glb[0, 0], glb[0, 1], glb[1, 3] = bm.FLOAT_MISSING_BITS, 0x7FC12345, 0x80000000
    ad = rng.integers(0, 40, (S, N * 5)).astype(np.int32)
    keys = [(1, "DP", "Integer"), (130, "PL", "Integer"), (40000, "GL", "Float"), (4, "AD", "Integer")]
    fields = [(1, dp, bm.ONE), (40000, gl, bm.PER_G), (130, pl, bm.PER_G), (4, ad, bm.PER_A)]
    data, off = bm.encode(fields, st, na, N)
    assert off[0] == 0 and off[-1] == len(data) and off[3] == off[4]  # the skipped site has no bytes
    kept = [i for i in range(S) if st[i] >= 0]
    write_bcf(str(tmp_path / "m.bcf"), N, keys, [(10 + i, ["A"] * int(na[i]), 4, data[off[i]:off[i + 1]]) for i in kept])
    recs = list(bcf_reader.Reader(str(tmp_path / "m.bcf")).records())
    assert len(recs) == len(kept)
    widths = set()
    for i, r in zip(kept, recs):
        nA = int(na[i]); nG = nA * (nA + 1) // 2
        assert r["pos0"] == 10 + i and len(r["alleles"]) == nA
        assert [k for k, _, _ in r["fmt"]] == ["DP", "GL", "PL", "AD"]
        for (name, t, per), (_, arr, kind) in zip(r["fmt"], fields):
            n = {bm.ONE: 1, bm.PER_G: nG, bm.PER_A: nA}[kind]
            want = arr[i, :n * N].reshape(N, n)
            if arr.dtype == np.float32:
                assert t == 5 and per == want.view(np.uint32).tolist()
            else:
                widths.add((name, t))
                assert per == [[None if v == M else "END" if v == E else int(v) for v in row] for row in want]
    assert {("PL", 1), ("PL", 2), ("PL", 3)} <= widths                # every integer width, and 15-value vectors among them
    assert any(len(per[0]) == 15 for r in recs for _, _, per in r["fmt"])


def host_hex(key, n, values):
    argv = [BIN, "--encode-ints", str(key), str(n)] + ["." if v == M else "e" if v == E else str(v) for v in values]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout.strip()


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
def test_model_equals_the_host_encoder_at_every_threshold():
    """both sides of 127 / 128, -120 / -121, 32767 / 32768, -32760 / -32761, INT32_MIN + 2, INT32_MAX, vectors without an ordinary value and
    mixed ones; key ids 0, 127, 128, 32767, 32768; n in {0, 1, 14, 15}"""
    cases = []
    for name, v in bm.threshold_vectors():
        cases.append((3, 1, v))
        cases.append((3, len(v), v))                                 # one sample of len(v) values
    for t in bm.THRESHOLDS:
        cases.append((9, 1, [t]))                                    # the threshold alone
    for key in (0, 127, 128, 32767, 32768):
        cases.append((key, 2, [1, 2, 300, M]))
    rng = np.random.default_rng(1)
    for n in (0, 1, 14, 15):
        cases.append((7, n, [int(x) for x in rng.integers(-100, 100, 2 * n)]))
        cases.append((7, n, [int(x) for x in rng.integers(-30000, 30000, 2 * n)]))
    types = set()
    for key, n, v in cases:
        want = bm.encode_int_field(key, n, v)
        assert host_hex(key, n, v) == want.hex(), (key, n, v)
        types.add(bm.int_type(v))
    assert types == {bm.BT_INT8, bm.BT_INT16, bm.BT_INT32}
    # the type at each threshold, spelled out
    for v, bt in ((127, 1), (128, 2), (-120, 1), (-121, 2), (32767, 2), (32768, 3), (-32760, 2), (-32761, 3), (M + 2, 3), (2 ** 31 - 1, 3)):
        assert bm.int_type([0, v]) == bt, v
    assert bm.int_type([M, M]) == bm.int_type([E]) == bm.int_type([]) == 1
    assert bm.encode_int_field(5, 0, []) == bytes([0x11, 5, 0x01])


def test_header_declares_the_bcf_entries():
    hdr = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert re.search(r"#define VGL_ABI_VERSION 7\b", hdr) and _abi.ABI_VERSION == 7
    for name in ENTRIES:
        assert re.search(r"VGL_API\s+\w+\s+" + name + r"\s*\(", hdr), name
        assert name in _abi.EXPORTS
    assert re.search(r"typedef struct vgl_bcf_field\s*\{", hdr)
    assert C.sizeof(_abi.BcfField) == 32
    assert [f for f, _ in _abi.BcfField._fields_] == ["key_id", "is_float", "count", "base", "site_stride"]


def test_bcfenc_is_a_submodule_only():
    import vcfgl_amd
    src = open(os.path.join(ROOT, "vcfgl_amd", "__init__.py")).read()
    assert "bcfenc" not in src
    from vcfgl_amd import bcfenc
    assert bcfenc.KEY_ORDER == ["DP", "GL", "PL", "GP", "AD", "ADF", "ADR"]
    assert (bcfenc.ONE, bcfenc.PER_G, bcfenc.PER_A) == (bm.ONE, bm.PER_G, bm.PER_A)


GVCF = ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1", "-doUnobserved", "2"]
# (argv, the flag the message names, what it says besides)
REFUSED = {
    "bad value": (["-O", "u", "--device-bcf", "2"], "--device-bcf", "Allowed range is [0,1]"),
    "vcf": (["-O", "v", "--device-bcf", "1"], "--device-bcf", "-O u or -O b"),
    "vcf.gz": (["-O", "z", "--device-bcf", "1"], "--device-bcf", "-O u or -O b"),
    "depth inf": (["-O", "b", "--device-bcf", "1", "--depth", "inf"], "--device-bcf", "--depth inf"),
    "gvcf on the host": (["-O", "u", "--device-bcf", "1"] + GVCF, "--device-bcf", "--device-gvcf 1"),
    "gvcf on the host, b": (["-O", "b", "--device-bcf", "1"] + GVCF, "--device-bcf", "--device-gvcf 1"),
    "vcf with both": (["-O", "v", "--device-bcf", "1", "--device-gvcf", "1"] + GVCF, "--device-bcf", "-O u or -O b"),
    # what was refused before stays refused, with its present message
    "device gvcf alone, u": (["-O", "u", "--device-gvcf", "1"] + GVCF, "--device-gvcf", "-O v or -O z"),
    "device gvcf alone, b": (["-O", "b", "--device-gvcf", "1"] + GVCF, "--device-gvcf", "-O v or -O z"),
    "device text, u": (["-O", "u", "--device-text", "1"], "--device-text", "-O v or -O z"),
    "device text, b": (["-O", "b", "--device-text", "1"], "--device-text", "-O v or -O z"),
    "device text with bcf": (["-O", "b", "--device-text", "1", "--device-bcf", "1"], "--device-text", "-O v or -O z"),
}


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refuses_device_bcf_where_it_cannot_apply(case, tmp_path):
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
    assert "--device-bcf 0|1" in r.stdout + r.stderr


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu() or not os.path.exists(BIN), reason="needs a machine WITHOUT a GPU and the built program")
def test_a_run_without_a_gpu_fails_and_does_not_fall_back(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", out, "-O", "u", "--seed", "1", "-e", "0.01", "--depth", "2", "--device-bcf", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no HIP device available" in r.stderr and "no CPU path" in r.stderr
    assert not os.path.exists(out + ".bcf") and "Simulation finished successfully" not in r.stderr
