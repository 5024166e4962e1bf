"""vcfgl_hip --device-inf without a GPU: the flag is opt-in (0 writes what no flag writes, through the host's --depth inf path, and
those records are the model's), everything it does not apply to is refused before a device is touched and before any file of the run
exists, the help text names it, and with 1 a machine without a GPU gets the library's message instead of a fallback.  Also the three
new entry points of the C ABI: declared, exported, and their argument checks that precede any device call."""
import os
import re
import subprocess

import pytest

import golden_util as gu
import inf_model as im
from vcfgl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(gu.REFVCF, "data", "data3.vcf")
DATA5 = os.path.join(gu.REFVCF, "data", "data5_acgt_multiallelic.vcf")
TAGS = ["-addGP", "1", "-addPL", "1"]
NEW = ["vgl_inf_workspace_bytes", "vgl_inf_fill_device", "vgl_ctx_true_values"]


def run(out, *flags, inp=DATA3):
    return subprocess.run([BIN, "-i", inp, "-o", out, "-O", "v", "--seed", "1", "-e", "0.01"] + list(flags), capture_output=True, text=True, timeout=120)


def refused(tmp_path, *flags):
    r = run(str(tmp_path / "out"), *flags)
    assert r.returncode == 1 and not any(f.startswith("out") for f in os.listdir(tmp_path)), r.stderr[-800:]
    return r.stderr


def body(path):
    return [ln for ln in open(path).read().split("\n") if ln and not ln.startswith("##source=")]


def test_it_needs_depth_inf_and_a_tag(tmp_path):
    err = refused(tmp_path, "-d", "3", "--device-inf", "1")
    assert "--device-inf 1" in err and "it needs --depth inf" in err
    err = refused(tmp_path, "-d", "inf", "--device-inf", "1", "-addGL", "0")
    assert "--device-inf 1 needs at least one of -addGL 1, -addGP 1 and -addPL 1" in err
    assert "Allowed range is [0,1]" in refused(tmp_path, "-d", "inf", "--device-inf", "2")


@pytest.mark.parametrize("flags,msg", [
    (["--gt-discordance", "1"], "--gt-discordance 1 is not supported with --depth inf (no tile is simulated: every call would be the truth)."),
    (["--fetch-gl", "AC"], "--fetch-gl AC is not supported with --depth inf (no tile is simulated)."),
    (["--set-alleles", "x.tsv"], "--set-alleles x.tsv is not supported with --depth inf (no tile is simulated: the records carry no likelihoods to relabel)."),
    (["--records", "0"], "--records 0 writes no record file: it needs --gt-discordance 1 or --fetch-gl XY"),
    (["--records", "0", "--gt-discordance", "1"], "--gt-discordance 1 is not supported with --depth inf"),
    (["--device-gvcf", "1", "-doGVCF", "1", "--gvcf-dps", "1"], "--device-gvcf 1 is not supported with --depth inf (no tile is simulated)."),
    (["-doGVCF", "1", "--gvcf-dps", "1"], "[-doGVCF 1] Cannot output gVCF when --depth inf is set."),
    (["-printPileup", "1"], "--device-inf 1 is not supported with -printPileup 1"),
    (["-printPileup", "1", "--device-pileup", "1"], "--device-inf 1 is not supported with -printPileup 1"),
    (["--rm-invar-sites", "4"], "[--rm-invar-sites 4] Cannot skip invariable sites when --depth inf is set."),
    (["-addQS", "1"], "(-addQS 1) QS tag cannot be added when --depth inf is set."),
    (["-addI16", "1"], "(-addI16 1) I16 tag cannot be added when --depth inf is set.")])
def test_what_stays_refused_with_the_flag(tmp_path, flags, msg):
    assert msg in refused(tmp_path, "-d", "inf", "--device-inf", "1", *TAGS, *flags)


@pytest.mark.parametrize("flags,msg", [
    (["--device-text", "1"], "--device-text 1 is not supported with --depth inf (no tile is simulated)."),
    (["--device-stream", "1"], "--device-stream 1 is not supported with --depth inf (no tile is simulated)."),
    (["-O", "u", "--device-bcf", "1"], "--device-bcf 1 is not supported with --depth inf (no tile is simulated)."),
    (["--device-input", "1"], "--device-input 1 is not supported with --depth inf (no device is used)."),
    (["--device-bcf-input", "1"], "--device-bcf-input 1 is not supported with --depth inf (no device is used)."),
    (["--device-inflate", "1"], "--device-inflate 1 is not supported with --depth inf (no device is used)."),
    (["--device-pileup", "1", "-printPileup", "1"], "--device-pileup 1 is not supported with --depth inf")])
@pytest.mark.parametrize("off", [[], ["--device-inf", "0"]])
def test_without_the_flag_every_refusal_is_todays(tmp_path, flags, msg, off):
    assert msg in refused(tmp_path, "-d", "inf", *TAGS, *off, *flags)


def test_flag_0_writes_what_no_flag_writes_and_both_are_the_model(tmp_path):
    for k, (inp, extra) in enumerate([(DATA3, ["-explode", "1", "-doUnobserved", "1"]), (DATA5, ["--source", "1", "-doUnobserved", "4"]),
                                      (DATA5, ["--source", "1", "-doUnobserved", "0", "-addGL", "0"])]):
        a, b = str(tmp_path / ("a%d" % k)), str(tmp_path / ("b%d" % k))
        ra = run(a, "-d", "inf", "-printTruth", "1", *TAGS, *extra, inp=inp)
        rb = run(b, "-d", "inf", "-printTruth", "1", "--device-inf", "0", *TAGS, *extra, inp=inp)
        assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr[-500:], rb.stderr[-500:])
        assert sorted(os.listdir(tmp_path)) == sorted(x + str(j) + e for j in range(k + 1) for x in "ab" for e in (".arg", ".truth.vcf", ".vcf"))
        assert body(a + ".vcf") == body(b + ".vcf") and body(a + ".truth.vcf") == body(b + ".truth.vcf")
        summary = lambda r: r.stderr[r.stderr.index("-> Simulation finished"):]
        assert summary(ra) == summary(rb) and "Total number of sites simulated" in summary(ra)
        # the host path's records against the model, from the genotypes its own truth file holds
        gt, where = im.read_vcf_gt(a + ".truth.vcf", source=1)
        d = int(extra[extra.index("-doUnobserved") + 1])
        keys = tuple(t for t in ("GL", "GP", "PL") if not (t == "GL" and "-addGL" in extra))
        want = im.record_columns(gt, d, keys=keys, nonref="<*>")
        got = [ln.split("\t") for ln in body(a + ".vcf") if not ln.startswith("#")]
        assert len(got) == len(want) == (10 if inp == DATA3 else 6)
        for (chrom, pos), (ref, alt, fmt, cols), g in zip(where, want, got):
            assert [chrom, str(pos), ref, alt, fmt] + cols == [g[0], g[1], g[3], g[4], g[8]] + g[9:]


def test_the_help_text_names_the_flag():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--device-inf 0|1" in r.stderr and "Needs --depth inf" in r.stderr


def test_without_a_gpu_flag_1_fails_with_the_librarys_message(tmp_path):
    # (HIP_VISIBLE_DEVICES=-1 hides the devices of a machine that has some: the same run everywhere)
    r = subprocess.run([BIN, "-i", DATA3, "-o", str(tmp_path / "out"), "-O", "v", "--seed", "1", "-e", "0.01", "-d", "inf", "--device-inf", "1"] + TAGS,
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "no HIP device available (this library has no CPU path)" in r.stderr and not os.path.exists(str(tmp_path / "out.vcf"))


def test_the_entry_points_are_declared_and_exported():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.EXPORTS
        assert re.search(r"VGL_API\s+\w+\s+%s\(" % name, header), name
    assert lib.vgl_abi_version() == _abi.ABI_VERSION == 7        # additive: the version stays
    assert len(_abi.EXPORTS) == len(set(_abi.EXPORTS)) == 89 == len(re.findall(r"^VGL_API\s", header, re.M))
    assert "exports the header's 89 entry points only" in open(os.path.join(ROOT, "README.md")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vcfgl_amd", "lib", "libvcfgl_hip.so")], capture_output=True, text=True, timeout=60).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("vgl_")}
    assert exported == set(_abi.EXPORTS)                         # (vgl_inf_fill_impl, the contexts' variant, is not exported)


def test_workspace_arithmetic_and_argument_checks():
    lib = _abi.load_library()
    ws = lib.vgl_inf_workspace_bytes
    for n, s in [(1, 1), (65, 37), (1000, 4096), (0, 0), (5, 0)]:
        assert ws(n, s) == (8 * s + 255) // 256 * 256             # one 8-byte map per site, rounded up to 256 bytes
    assert ws(-1, 1) == ws(1, -1) == -1
    p = 4096                                                     # never dereferenced: every case fails its check first
    #     device N  S  doU G   A  layout                 gt st na no a2b gl    pl    gp    u8    bad ws ws_bytes stream
    ok = [0, 1, 1, 1, 15, 5, _abi.VGL_LAYOUT_PLANES, p, p, p, p, p, None, None, None, None, p, p, 1 << 20, None]
    cases = [(1, 0), (1, -3), (2, -1), (3, -1), (3, 6), (4, 10), (5, 4), (6, 2), (6, -1), (7, None), (8, None), (9, None), (10, None), (11, None),
             (16, None), (17, None), (18, 7), (18, -1)]
    for k, v in cases:
        a = list(ok)
        a[k] = v
        assert lib.vgl_inf_fill_device(*a) == _abi.VGL_E_ARG, (k, v)
        assert b"vgl_inf_fill_device" in lib.vgl_last_error()
    for d, g, al in [(0, 15, 5), (3, 15, 5), (1, 10, 4), (4, 10, 4), (5, 10, 5), (2, 15, 4)]:      # a pair that do_unobserved does not give
        a = list(ok)
        a[3:6] = [d, g, al]
        assert lib.vgl_inf_fill_device(*a) == _abi.VGL_E_ARG, (d, g, al)
    a = list(ok)
    a[2] = 0                                                     # no sites: nothing to do, nothing is looked at
    a[7:12] = [None] * 5
    assert lib.vgl_inf_fill_device(*a) == _abi.VGL_OK
    assert lib.vgl_ctx_true_values(None, 1) == _abi.VGL_E_ARG
