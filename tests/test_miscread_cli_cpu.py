"""--device-inflate of the three misc programs and --resident of fetchgl_hip, as far as a machine without a GPU shows them: the help
texts, the refusals at parse time, and the clean failure of --device-inflate 1 without a device (exit 1, the library's text, no
output file).  What the flags compute is tests/test_gpu_miscread.py and tests/test_gpu_resident.py."""
import os
import subprocess

import pytest

import fgl_file_model as gm
import sal_file_model as sm
from vcfgl_amd import discordance as D
from vcfgl_amd import fetchgl as F
from vcfgl_amd import setalleles as S

NO_DEVICE = "no HIP device is available"


HIDDEN = dict(os.environ, HIP_VISIBLE_DEVICES="-1")      # a machine with a GPU shows none


def _help(program):
    r = subprocess.run([program, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    return r.stderr


def test_the_help_of_each_program_lists_the_new_flags():
    for program in (F.FETCHGL_PROGRAM, S.SETALLELES_PROGRAM, D.GTDISC_PROGRAM):
        text = _help(program)
        assert "--device-inflate 0|1 [0]" in text and "opens the GPU under --on-device 0" in text
    text = _help(F.FETCHGL_PROGRAM)
    assert "--resident 0|1 [0]" in text and "--resident-max-bytes INT" in text
    for program in (S.SETALLELES_PROGRAM, D.GTDISC_PROGRAM):
        assert "--resident" not in _help(program)


@pytest.fixture(scope="module")
def bgz(tmp_path_factory):
    d = tmp_path_factory.mktemp("miscread_cpu")
    recs = gm.make_records(3, 5, seed=1, fixed_alleles=True)
    return gm.write_file(str(d / "in.bgz"), recs, 3, "bgz")


def test_resident_needs_both_other_flags(bgz):
    for kw in (dict(on_device=True), dict(on_device=True, device_inflate=False), dict(on_device=False, device_inflate=True), dict(on_device=False)):
        rc, so, se = F.fetch_file(bgz, "AC", resident=True, timeout=60, **kw)
        assert rc == 1 and so == "" and "--resident 1 needs --device-inflate 1 and --on-device 1" in se, se
    rc, so, se = F.fetch_file(bgz, "AC", on_device=False, resident=False, timeout=60)
    assert rc == 0 and so.count("\n") == 5


def test_values_outside_0_and_1_are_refused(bgz):
    for flag in ("--device-inflate", "--resident"):
        r = subprocess.run([F.FETCHGL_PROGRAM, "-i", bgz, "-gt", "AC", "--on-device", "0", flag, "2"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and flag + " takes an integer in 0 .. 1" in r.stderr
    for program, args in ((S.SETALLELES_PROGRAM, ["-i", bgz, "-a", bgz]), (D.GTDISC_PROGRAM, ["-i", bgz, "-t", bgz, "-o", os.devnull])):
        r = subprocess.run([program] + args + ["--on-device", "0", "--device-inflate", "2"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--device-inflate takes an integer in 0 .. 1" in r.stderr
    r = subprocess.run([F.FETCHGL_PROGRAM, "-i", bgz, "-gt", "AC", "--resident-max-bytes", "-1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--resident-max-bytes takes an integer of at least 0" in r.stderr


def test_device_inflate_without_a_gpu_fails_before_the_output_is_opened(bgz, tmp_path):
    out = str(tmp_path / "out.csv")
    rc, so, se = F.fetch_file(bgz, "AC", out=out, on_device=False, device_inflate=True, timeout=60, env=HIDDEN)
    assert rc == 1 and so == "" and NO_DEVICE in se and "--device-inflate 1" in se and not os.path.exists(out)
    # the file is looked for first, as with 0
    rc, so, se = F.fetch_file(str(tmp_path / "none.bgz"), "AC", on_device=False, device_inflate=True, timeout=60, env=HIDDEN)
    assert rc == 1 and "Could not open file" in se
    rc, so, se = F.fetch_file(str(tmp_path / "none.bgz"), "AC", on_device=True, device_inflate=True, resident=True, timeout=60, env=HIDDEN)
    assert rc == 1 and "Could not open file" in se and NO_DEVICE not in se          # --resident 1 too
    rc, so, se = F.fetch_file(bgz, "AC", out=out, on_device=True, device_inflate=True, resident=True, timeout=60, env=HIDDEN)
    assert rc == 1 and so == "" and NO_DEVICE in se and not os.path.exists(out)
    recs = sm.make_records(3, 5, seed=2, tags="GL")
    path, tsv, prefix = str(tmp_path / "s.vcf.gz"), str(tmp_path / "s.tsv"), str(tmp_path / "sout")
    sm.write_file(path, sm.vcf_text(recs, 3), "bgz")
    open(tsv, "w").write(sm.tsv_text(recs))
    rc, so, se = S.set_file(path, tsv, prefix, "v", on_device=False, device_inflate=True, timeout=60, env=HIDDEN)
    assert rc == 1 and NO_DEVICE in se and not os.path.exists(prefix + ".vcf")
    assert S.set_file(path, tsv, prefix, "v", on_device=False, device_inflate=False, timeout=60)[0] == 0 and os.path.exists(prefix + ".vcf")
    out = str(tmp_path / "d.tsv")
    rc, so, se = D.compare_files(bgz, bgz, out, on_device=False, device_inflate=True, timeout=60, env=HIDDEN)
    assert rc == 1 and NO_DEVICE in se and not os.path.exists(out)
