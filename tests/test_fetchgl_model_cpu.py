"""The model of misc/fetchGl (tests/fetchgl_model.py) against what the reference recorded, its per-value %f against exact rational
arithmetic, and the pure-host arithmetic of the library's fetch-GL entry points."""
import os
import subprocess

import numpy as np
import pytest

import fetchgl_model as fm
from vcfgl_amd import _abi, fetchgl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_fetchgl")


def _read(*p):
    return open(os.path.join(*p)).read()


def test_model_reproduces_the_recorded_output_of_test12():
    assert fm.file_lines(_read(GOLD, "data", "test12.vcf"), "CC") == _read(GOLD, "reference", "test12.csv")


def test_model_reproduces_the_readme_listing_of_test10():
    got = fm.file_lines(_read(ROOT, "tests", "golden", "ref_vcf", "reference", "test10", "test10.vcf"), "AC")
    head = _read(GOLD, "reference", "test10_AC_head.csv")
    assert got.startswith(head) and len(got.splitlines()) == 10 and len(head.splitlines()) == 8


def test_percent_f_is_exact_half_even_rounding():
    """every exact tie of the sixth decimal (odd k 2^-7), its neighbours, the carries: Python's %f against fractions.Fraction"""
    pats = fm.value_set(n_random=2000)
    n = 0
    for b in pats:
        b = int(b)
        if (b & 0x7FFFFFFF) >= 0x7F800000:
            continue
        assert fm.fmt_value_bits(b, fm.FLOAT) == fm.exact_f(b), hex(b)
        n += 1
    assert n > 10000
    assert fm.fmt_value_bits(fm._f32(0.0078125), fm.FLOAT) == "0.007812" and fm.fmt_value_bits(fm._f32(0.0234375), fm.FLOAT) == "0.023438"
    assert fm.fmt_value_bits(fm._f32(-1e-9), fm.FLOAT) == "-0.000000" and fm.fmt_value_bits(0x80000000, fm.TEXT) == "-0.000000"


def test_the_two_value_modes_differ_where_the_text_has_fewer_digits():
    b = fm._f32(-123.457)
    assert fm.fmt_value_bits(b, fm.TEXT) == "-123.457001" == fm.fmt_value_bits(b, fm.FLOAT)
    b = fm._f32(-123.45678)
    assert fm.fmt_value_bits(b, fm.FLOAT) == "-123.456779" and fm.fmt_value_bits(b, fm.TEXT) == "-123.457001"
    assert fm.fmt_value_bits(fm.MISSING_BITS, fm.TEXT) == fm.fmt_value_bits(fm.MISSING_BITS, fm.FLOAT) == "MISSING"
    assert fm.fmt_value_bits(fm.END_BITS, fm.FLOAT) == "END" and fm.fmt_value_bits(fm.END_BITS, fm.TEXT) == "nan"
    assert fm.fmt_value_bits(0xFFC00000, fm.FLOAT) == "-nan" and fm.fmt_value_bits(0xFFC00000, fm.TEXT) == "nan"
    assert fm.fmt_value_bits(0xFF800000, fm.TEXT) == "-inf" and fm.fmt_value_bits(0x7F800000, fm.FLOAT) == "inf"
    big = fm._f32(1e22)
    assert fm.fmt_value_bits(big, fm.TEXT) == fm.fmt_value_bits(big, fm.FLOAT) == fm.exact_f(big)
    assert len(fm.fmt_value_bits(0xFF7FFFFF, fm.FLOAT)) == 47


def test_bound_and_workspace_arithmetic():
    lib = _abi.load_library()
    for n, s in ((1, 1), (1000, 32768), (257, 7), (0, 5), (5, 0)):
        assert lib.vgl_fetchgl_bound(n, s) == n * s * 48 == fetchgl.bound(n, s)
        assert lib.vgl_fetchgl_workspace_bytes(n, s) == n * s * 4
    assert lib.vgl_fetchgl_bound(2 ** 31 - 1, 2 ** 25) == (2 ** 31 - 1) * 2 ** 25 * 48
    assert lib.vgl_fetchgl_bound(2 ** 31 - 1, 2 ** 31 - 1) == -1                      # beyond int64
    for n, s in ((-1, 1), (1, -1)):
        assert lib.vgl_fetchgl_bound(n, s) == -1 and lib.vgl_fetchgl_workspace_bytes(n, s) == -1


def test_lines_prefixes_pos_to_every_non_empty_site():
    text = b"a,b\n" + b"MISSING\n"
    off = np.array([0, 0, 4, 4, 12, 12], dtype=np.int64)
    assert fetchgl.lines([5, 6, 7, 9, 11], text, off) == b"6,a,b\n9,MISSING\n" == fm.lines([5, 6, 7, 9, 11], text, off)
    assert fetchgl.allele_codes("A<") == (0, 4) and fetchgl.allele_codes("TC") == (3, 1)
    for bad in ("A", "ACG", "AN", "a<", ""):
        try:
            fetchgl.allele_codes(bad)
        except ValueError:
            continue
        raise AssertionError(bad)


BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data")


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("flags,names", [
    (["--fetch-gl", "AN"], ["--fetch-gl"]),
    (["--fetch-gl", "A"], ["--fetch-gl"]),
    (["--fetch-gl", "ACG"], ["--fetch-gl"]),
    (["--fetch-gl", "ac"], ["--fetch-gl"]),
    (["--fetch-gl", "AC", "--depth", "inf"], ["--fetch-gl", "--depth inf"]),
    (["--fetch-gl", "AC", "-doGVCF", "1"], ["--fetch-gl", "-doGVCF"]),
    (["--fetch-gl", "AC", "-addGL", "0", "-addPL", "1"], ["--fetch-gl", "-addGL", "Could not read GL tag"]),
    (["--fetch-gl-value", "1"], ["--fetch-gl-value", "--fetch-gl"]),
    (["--fetch-gl", "AC", "--fetch-gl-value", "3"], ["--fetch-gl-value"]),
    (["--records", "0"], ["--records", "--gt-discordance", "--fetch-gl"]),
    (["--fetch-gl", "AC", "--records", "0", "-printTruth", "1"], ["--records", "-printTruth"]),
])
def test_binary_refuses_before_it_touches_a_device(flags, names, tmp_path):
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", str(tmp_path / "o"), "--seed", "1", "-e", "0.01"]
    if "--depth" not in flags:
        argv += ["--depth", "2"]
    r = subprocess.run(argv + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    for name in names:
        assert name in r.stderr, r.stderr
    assert "HIP device" not in r.stderr and not os.path.exists(str(tmp_path / "o") + ".fetchgl.csv")


def test_help_documents_both_flags():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert "--fetch-gl XY" in r.stdout + r.stderr and "--fetch-gl-value 0|1|2" in r.stdout + r.stderr
