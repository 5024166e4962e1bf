"""The split BCF reader of the host program under AddressSanitizer + UBSan, without a GPU: truncations and seeded byte mutations of
valid BCF files through --dump-gt FILE 1 3 (the reader, the shared per-sample rule on each record's GT slice, make_site) and through
a --depth inf run with the flag off.  A damaged input must end in an error message or in a clean run, never in a sanitizer report.
(Sanitizers are not available on the GPU pool; the device path is covered by the -m gpu tests.)"""
import os
import random
import subprocess

import pytest

import bcfin_cases as bc
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
LIB = os.path.join(ROOT, "vcfgl_amd", "lib")
DATA = os.path.join(gu.REFVCF, "data")
SAN_MARKS = ("AddressSanitizer", "runtime error", "LeakSanitizer")


@pytest.fixture(scope="module")
def asan_bin(tmp_path_factory):
    if not os.path.exists(os.path.join(LIB, "libvcfgl_hip.so")):
        subprocess.check_call(["make", "-C", CSRC, "all"])
    out = str(tmp_path_factory.mktemp("asan") / "vcfgl_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(CSRC, "host", "vcfgl_main.cpp"),
                           "-L" + LIB, "-lvcfgl_hip", "-lz", "-pthread", "-Wl,-rpath," + LIB])
    return out


@pytest.fixture(scope="module")
def sources(asan_bin, tmp_path_factory):
    """valid BCFs: the program's own truth output of a multiallelic golden input, and the hand-built file of odd records"""
    d = tmp_path_factory.mktemp("src")
    r = subprocess.run([asan_bin, "-i", os.path.join(DATA, "data5_acgt_multiallelic.vcf"), "-o", str(d / "seed"), "-O", "u", "--source", "1",
                        "--seed", "1", "--depth", "inf", "-e", "0", "-printTruth", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not any(m in r.stderr for m in SAN_MARKS), r.stderr[-2000:]
    return [open(str(d / "seed") + ".truth.bcf", "rb").read(), bc.odd_bcf()[0]]


def both_ways(binary, path, tmp_path):
    """the hook with the device's statuses, and a --depth inf run with the flag off; returns the two exit codes"""
    out = []
    for argv in (["--dump-gt", path, "1", "3"],
                 ["-i", path, "-o", str(tmp_path / "out"), "--seed", "1", "--depth", "inf", "-e", "0", "-O", "v", "--source", "1", "--device-bcf-input", "0"]):
        r = subprocess.run([binary] + argv, capture_output=True, text=True, errors="replace", timeout=60)
        assert not any(m in r.stderr or m in r.stdout for m in SAN_MARKS), r.stderr[-3000:]
        assert r.returncode in (0, 1), (argv, r.returncode, r.stderr[-500:])
        assert r.returncode == 0 or "ERROR" in r.stderr + r.stdout
        out.append(r.returncode)
    return out


def test_valid_files_run_clean(asan_bin, sources, tmp_path):
    for k, src in enumerate(sources):
        f = str(tmp_path / ("ok%d.bcf" % k))
        open(f, "wb").write(src)
        # (--depth inf needs complete genotypes: the odd records, with their missing alleles, end in that message)
        assert both_ways(asan_bin, f, tmp_path) == [0, 0 if k == 0 else 1]


def test_truncated_files(asan_bin, sources, tmp_path):
    """cut at the end of the header, inside the first record's lengths, shared block and FORMAT fields, and at 40 seeded places"""
    rng = random.Random(11)
    f = str(tmp_path / "cut.bcf")
    for src in sources:
        hdr_end = 9 + int.from_bytes(src[5:9], "little")
        l_shared = int.from_bytes(src[hdr_end:hdr_end + 4], "little")
        cuts = [3, 8, hdr_end - 1, hdr_end, hdr_end + 3, hdr_end + 7, hdr_end + 8 + 10, hdr_end + 8 + l_shared, hdr_end + 8 + l_shared + 2, len(src) - 1]
        cuts += [rng.randrange(hdr_end, len(src)) for _ in range(40)]
        failed = 0
        for n in cuts:
            open(f, "wb").write(src[:n])
            rc = both_ways(asan_bin, f, tmp_path)
            failed += rc[0] != 0
        assert failed >= len(cuts) // 2                                  # (a cut between two records leaves a valid, shorter file)


def test_random_mutations(asan_bin, sources, tmp_path):
    rng = random.Random(20260101)
    f = str(tmp_path / "mut.bcf")
    for src in sources:
        hdr_end = 9 + int.from_bytes(src[5:9], "little")
        for k in range(120):
            b = bytearray(src)
            for _ in range(rng.randint(1, 4)):
                i = rng.randrange(5, len(b)) if rng.random() < 0.3 else rng.randrange(hdr_end, len(b))   # mostly inside the records
                if rng.random() < 0.7:
                    b[i] = rng.choice((rng.randrange(256), 0x80, 0x81, 0xFF, 0x7F))
                else:
                    del b[i:i + rng.randint(1, 9)]
            open(f, "wb").write(bytes(b))
            both_ways(asan_bin, f, tmp_path)
