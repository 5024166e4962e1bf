"""--resident-bcf of fetchgl_hip as far as a machine without a GPU shows it: the help text, the refusals at parse time, the clean
failure without a device (exit 1, no output file), and a run with the flag at 0, which is the run without it.  What the flag computes
is tests/test_gpu_resident_bcf.py."""
import os
import subprocess

import pytest

import fgl_file_model as gm
from vcfgl_amd import fetchgl as F

NO_DEVICE = "no HIP device is available"
HIDDEN = dict(os.environ, HIP_VISIBLE_DEVICES="-1")      # a machine with a GPU shows none


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("residentbcf_cpu")
    recs = gm.make_records(3, 5, seed=1, fixed_alleles=True)
    raw = gm.bcf_bytes(recs, 3)
    bcf, bgz = str(d / "in.bcf"), str(d / "in.bcf.bgz")
    open(bcf, "wb").write(raw)
    open(bgz, "wb").write(gm.bgzf(raw))
    return bcf, bgz


def test_the_help_lists_the_flag():
    r = subprocess.run([F.FETCHGL_PROGRAM, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--resident-bcf 0|1 [0]" in r.stderr and "--resident 0|1 [0]" in r.stderr
    assert "1: a BGZF file of VCF text stays in GPU memory once inflated" in r.stderr       # --resident keeps its own help text


def test_it_needs_resident_1_and_says_so(files):
    bcf, bgz = files
    for kw in (dict(), dict(resident=False), dict(device_inflate=True), dict(on_device=False)):
        rc, so, se = F.fetch_file(bgz, "AC", resident_bcf=True, timeout=60, **kw)
        assert rc == 1 and so == "" and "--resident-bcf 1 needs --resident 1" in se, se
    # --resident 1 keeps its own needs
    rc, so, se = F.fetch_file(bgz, "AC", resident=True, resident_bcf=True, timeout=60)
    assert rc == 1 and "--resident 1 needs --device-inflate 1 and --on-device 1" in se


def test_a_value_of_2_is_refused(files):
    r = subprocess.run([F.FETCHGL_PROGRAM, "-i", files[1], "-gt", "AC", "--on-device", "0", "--resident-bcf", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--resident-bcf takes an integer in 0 .. 1" in r.stderr


def test_without_a_gpu_the_run_fails_before_the_output_is_opened(files, tmp_path):
    out = str(tmp_path / "out.csv")
    rc, so, se = F.fetch_file(files[1], "AC", out=out, on_device=True, device_inflate=True, resident=True, resident_bcf=True, timeout=60, env=HIDDEN)
    assert rc == 1 and so == "" and NO_DEVICE in se and not os.path.exists(out)
    rc, so, se = F.fetch_file(str(tmp_path / "none.bgz"), "AC", on_device=True, device_inflate=True, resident=True, resident_bcf=True, timeout=60, env=HIDDEN)
    assert rc == 1 and "Could not open file" in se and NO_DEVICE not in se


def test_with_0_a_raw_bcf_gives_the_csv_of_today(files):
    bcf, _ = files
    want = gm.run_file(bcf, "AC")
    base = F.fetch_file(bcf, "AC", on_device=False, timeout=60)
    got = F.fetch_file(bcf, "AC", on_device=False, resident=False, resident_bcf=False, timeout=60)
    assert got == base and got[0] == 0 and got[1] == "".join(want.stdout) and got[2] == "".join(want.messages)
    assert got[1].count("\n") == 5
