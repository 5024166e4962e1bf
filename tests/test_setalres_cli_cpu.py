"""setalleles_hip --resident on the command line, no GPU touched: the refusals of --resident 1 without --device-inflate 1 or without
--on-device 1 and of a bad --resident-max-bytes (a message, exit status 1, no output file), the bound of a resident batch in -h, the
command line the Python wrapper builds, and --resident 0 on the tool's two recorded outputs: the same bytes and the same stderr as without the flag."""
import os
import subprocess

import pytest

import sal_file_model as M
from vcfgl_amd import setalleles as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_setalleles")
DATA2 = os.path.join(GOLD, "data", "data2.vcf")
TSV1 = os.path.join(GOLD, "data", "data2_alleles1.tsv")


def program(*args):
    r = subprocess.run([S.SETALLELES_PROGRAM] + list(args), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--resident", "1"], "--resident 1 needs --device-inflate 1 and --on-device 1."),
    (["--resident", "1", "--device-inflate", "0", "--on-device", "1"], "--resident 1 needs --device-inflate 1 and --on-device 1."),
    (["--resident", "1", "--device-inflate", "1", "--on-device", "0"], "--resident 1 needs --device-inflate 1 and --on-device 1."),
    (["--resident", "2"], "--resident takes an integer in 0 .. 1, not '2'"),
    (["--resident-max-bytes", "-1"], "--resident-max-bytes takes an integer of at least 0, not '-1'"),
    (["--resident-max-bytes", "12x"], "--resident-max-bytes takes an integer of at least 0, not '12x'"),
    (["--resident-max-bytes", "x"], "--resident-max-bytes takes an integer of at least 0, not 'x'"),
])
def test_refusals_come_before_the_output_is_opened(tmp_path, flags, word):
    prefix = str(tmp_path / "out")
    rc, so, se = program("-i", DATA2, "-a", TSV1, "-O", "v", "-o", prefix, *flags)
    assert rc == 1 and so == "" and word in se and "finished" not in se
    assert not os.path.exists(prefix + ".vcf") and not os.path.exists(prefix + ".bcf")


def test_the_refusal_has_the_wording_of_fetchgl_hip():
    fetch = os.path.join(os.path.dirname(S.SETALLELES_PROGRAM), "fetchgl_hip")
    r = subprocess.run([fetch, "-i", DATA2, "-gt", "AA", "--resident", "1"], capture_output=True, text=True, timeout=120)
    rc, so, se = program("-i", DATA2, "-a", TSV1, "-o", "unused", "--resident", "1")
    assert r.returncode == 1 and rc == 1
    line = [ln for ln in se.splitlines() if "--resident 1 needs" in ln]
    assert line and line == [ln for ln in r.stderr.splitlines() if "--resident 1 needs" in ln]


def test_help_states_the_bound_of_a_resident_batch():
    """(the flags themselves are described in README.md: tests/test_miscread_cli_cpu.py holds this help text to be without them)"""
    rc, so, se = program("-h")
    assert rc == 0 and "64 MiB of assembled records" in se and "a larger record is a batch of its own" in se


def test_the_wrappers_command_line(monkeypatch, tmp_path):
    seen = []

    class Done:
        returncode, stdout, stderr = 0, "", ""

    monkeypatch.setattr(S.subprocess, "run", lambda cmd, **kw: seen.append(cmd) or Done())
    S.set_file("in.bcf", "a.tsv", "out", "b", device_inflate=True, resident=True, resident_max_bytes=123456789012, batch_records=7)
    S.set_file("in.bcf", "a.tsv", "out", "u", resident=False)
    S.set_file("in.bcf", "a.tsv", "out", "u")
    tail = seen[0][seen[0].index("--on-device"):]
    assert tail == ["--on-device", "1", "--batch-records", "7", "--device-inflate", "1", "--resident", "1", "--resident-max-bytes", "123456789012"]
    assert seen[1][-2:] == ["--resident", "0"] and "--resident-max-bytes" not in seen[1]
    assert "--resident" not in seen[2] and "--resident-max-bytes" not in seen[2]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("mode", ["v", "z"])
def test_resident_0_writes_the_recorded_outputs(tmp_path, k, mode):
    tsv = os.path.join(GOLD, "data", "data2_alleles%d.tsv" % k)
    with_flag, without = str(tmp_path / "with"), str(tmp_path / "without")
    ext = {"v": ".vcf", "z": ".vcf.gz"}[mode]
    a = S.set_file(DATA2, tsv, with_flag, mode, on_device=False, verbose=True, resident=False, resident_max_bytes=1, timeout=120)
    b = S.set_file(DATA2, tsv, without, mode, on_device=False, verbose=True, timeout=120)
    want = open(os.path.join(GOLD, "reference", "data2_alleles%d.vcf" % k), "rb").read()
    assert a[0] == 0 and b[0] == 0 and M.read_output(with_flag + ext) == want and M.read_output(without + ext) == want
    fields = lambda se, p: se.replace(p, "P").split("; read ")[0]                          # (the times differ from run to run)
    assert fields(a[2], with_flag) == fields(b[2], without) and "resident" not in a[2].replace(with_flag, "P")
    assert a[2].count("\n") == b[2].count("\n")


def test_resident_0_on_generated_bcf_is_the_same_file(tmp_path):
    recs = M.make_records(9, 12, seed=5, wide_pl=True)
    path, tsv = str(tmp_path / "in.bcf"), str(tmp_path / "in.tsv")
    M.write_bcf(path, M.bcf_records(recs, 9, end_every=5), 9, "bcf.gz")
    open(tsv, "w").write(M.tsv_text(recs))
    for mode in ("u", "b"):
        a = S.set_file(path, tsv, str(tmp_path / "a"), mode, on_device=False, resident=False, timeout=120)
        b = S.set_file(path, tsv, str(tmp_path / "b"), mode, on_device=False, timeout=120)
        assert a[0] == 0 and b[0] == 0
        assert open(str(tmp_path / "a.bcf"), "rb").read() == open(str(tmp_path / "b.bcf"), "rb").read()
