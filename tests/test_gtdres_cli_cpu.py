"""gtdiscordance_hip --resident as far as a machine without a GPU shows it: the refusals at parse time, a help text that does not
list the flag, the clean failure without a device (exit 1, the no-device message, no output file; a missing input file is reported
first), --resident 0 on the reference's own pairs, and the any-address 16-byte load of the decode kernel (gtd::load16_any of
vcfgl_amd/csrc/misc/gtdres_core.h) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  What the flag
computes is tests/test_gpu_gtdres.py."""
import os
import subprocess

import pytest

import gtdbcf_cases as gc
import gtdisc_model as gm
from vcfgl_amd import discordance as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "misc_gtdiscordance")
g = lambda name: os.path.join(GOLD, "data", name)
ref = lambda name: open(os.path.join(GOLD, "reference", name)).read()
NO_DEVICE = "no HIP device is available"
HIDDEN = dict(os.environ, HIP_VISIBLE_DEVICES="-1")      # a machine with a GPU shows none


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtdres_cpu")
    t, c = str(d / "t.vcf"), str(d / "c.vcf")
    gm.write_pair(t, c, 3, 5, "GT:GQ", seed=1)
    tz, cz = str(d / "t.vcf.gz"), str(d / "c.vcf.gz")
    for src, dst in ((t, tz), (c, cz)):
        with open(dst, "wb") as f:
            f.write(gc.bgzf(open(src, "rb").read()))
    return tz, cz


def test_resident_needs_both_other_flags(pair, tmp_path):
    tz, cz = pair
    out = str(tmp_path / "out.tsv")
    for kw in (dict(on_device=True), dict(on_device=True, device_inflate=False), dict(on_device=False, device_inflate=True), dict(on_device=False)):
        rc, so, se = D.compare_files(tz, cz, out, resident=True, timeout=60, **kw)
        assert rc == 1 and so == "" and "--resident 1 needs --device-inflate 1 and --on-device 1." in se, se
        assert not os.path.exists(out)
    rc, so, se = D.compare_files(tz, cz, out, on_device=False, resident=False, timeout=60)
    assert rc == 0 and os.path.getsize(out) > 0


def test_values_outside_their_range_are_refused(pair):
    tz, cz = pair
    base = [D.GTDISC_PROGRAM, "-t", tz, "-i", cz, "-o", os.devnull, "--on-device", "0"]
    for v in ("2", "-1", "x"):
        r = subprocess.run(base + ["--resident", v], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--resident takes an integer in 0 .. 1" in r.stderr
    for v in ("-1", "x", ""):
        r = subprocess.run(base + ["--resident-max-bytes", v], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--resident-max-bytes takes an integer of at least 0" in r.stderr
    r = subprocess.run(base + ["--resident-max-bytes", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_the_help_does_not_list_the_flag():
    r = subprocess.run([D.GTDISC_PROGRAM, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--bcf-direct 0|1 [0]" in r.stderr and "--resident" not in r.stderr


def test_without_a_gpu_the_run_fails_before_the_output_is_opened(pair, tmp_path):
    tz, cz = pair
    out = str(tmp_path / "out.tsv")
    kw = dict(on_device=True, device_inflate=True, resident=True, timeout=60, env=HIDDEN)
    rc, so, se = D.compare_files(tz, cz, out, **kw)
    assert rc == 1 and so == "" and NO_DEVICE in se and "--resident 1" in se and not os.path.exists(out)
    # the file is looked for first, as without the flag: the truth file, then the call file
    none = str(tmp_path / "none.vcf.gz")
    rc, so, se = D.compare_files(none, cz, out, **kw)
    assert rc == 1 and "Could not open file: " + none in se and NO_DEVICE not in se and not os.path.exists(out)
    rc, so, se = D.compare_files(tz, none, out, **kw)
    assert rc == 1 and NO_DEVICE in se and not os.path.exists(out)      # (the truth file asks for the device before the call file is looked for)


@pytest.mark.parametrize("truth,call,mode,want", [("truth.vcf", "call.vcf", 0, "test_doGq0.tsv"), ("truth3.vcf", "call3.vcf", 7, "test3_doGq7.tsv"),
                                                  ("truth3.vcf", "call3_nogq_withpl.vcf", 8, "test3_doGq7.tsv"),
                                                  ("truth3.vcf", "call3_nogq_withpl_unobservedAllele.vcf", 8, "test3_doGq7.tsv")])
def test_resident_0_on_the_golden_pairs(truth, call, mode, want, tmp_path):
    out = str(tmp_path / "out.tsv")
    rc, so, se = D.compare_files(g(truth), g(call), out, do_gq=mode, on_device=False, resident=False, resident_max_bytes=0, timeout=120)
    assert rc == 0 and open(out).read() == ref(want) and so == "", se[-1000:]


def test_joined_loads_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gtdres_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "gtdres_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    loads, joined, refused = (int(x) for x in r.stdout.split()[1::2])
    # 16 places of the side x 41 distances x 96 starts; a joined load needs 16 bytes behind the first piece, so some are refused
    assert loads + refused == 16 * 41 * 96 and joined > 30000 and refused > 5000
