"""Randomised differential test of vcfgl_hip's device stages and side channels: every configuration tests/cli_stage_cases.py draws
(random input in four containers, random reference flags, a random admissible subset of --device-text / -bcf / -stream / -bgzf / -gvcf /
-pileup / -input / -inflate / -bcf-input / -inf and --records 0, random --tile-sites / --devices / thread counts; --set-alleles,
--fetch-gl and --gt-discordance requests) against its host twin -- the same run with every stage flag at 0 on one device and one tile
size -- in both RNG modes: exit status, the record file, the truth file, the pileup, the discordance table, the fetched GLs, stdout,
and for a refused run its message must be equal.  The host path is the specification (tests/test_gpu_cli_fuzz.py holds it against
the CPU oracle); the kernels' shapes are held by their own tests: this one covers the composition of the stages and the code between
the kernels and the files.

A case both runs refuse with the same message (the reference flags: a quality score outside --qs-bins, VGL_E_ADJQ) is counted and
skipped, and at most one in ten may be; a run refused with a message that names a stage flag is a failure of the generator's table or
of the program.  The input stages must have done their work on the device: the [input] lines of --verbose 1 say so.

One child process at a time, each under a timeout; after a process that faulted, aborted or ran out of time nothing more is started.
VGL_STAGE_FUZZ_CHUNKS / VGL_STAGE_FUZZ_SEED give longer one-off runs.

First run on one MI355X, the 16 fixed chunks (24 processes each): the slowest chunk took 10.1 s (chunk 10), the others 5.9 to 9.7 s,
135 s together; 94 of the 96 configurations ran in each RNG mode and 2 were refused by both paths (a quality score outside
--qs-bins); 58 different stage subsets were seen; no difference was found."""
import collections
import json
import os
import re
import subprocess
import time

import pytest

import cli_stage_cases as sc

pytestmark = pytest.mark.gpu
CHUNKS = int(os.environ.get("VGL_STAGE_FUZZ_CHUNKS", str(sc.CHUNKS)))
SEED = int(os.environ.get("VGL_STAGE_FUZZ_SEED", str(sc.SEED)))
TIMEOUT = 120
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started
_seen = collections.Counter()          # runs per RNG mode, refusals, stage combinations, seconds per chunk


def _run(argv):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout: " + " ".join(argv))
        pytest.fail("vcfgl_hip ran out of time: no further GPU process is started\n" + " ".join(argv))
    if r.returncode in (-6, -11, 134, 139, 124, 137):
        _gave_up.append("status %d: %s" % (r.returncode, " ".join(argv)))
        pytest.fail("vcfgl_hip ended with status %d: no further GPU process is started\n%s\n%s" % (r.returncode, " ".join(argv), r.stderr[-1500:]))
    return r


def _pair(case, rng_mode, tmp, name):
    """the case and its host twin in one RNG mode: (artifacts of the device run, of the twin, the two results, the two argv lists)"""
    dev, host = str(tmp / ("dev_" + name)), str(tmp / ("host_" + name))
    av, ah = case.argv(dev, rng_mode), sc.host_twin(case).argv(host, rng_mode)
    rh, rv = _run(ah), _run(av)
    return (sc.artifacts(dev, case.mode, rv.returncode, rv.stdout, rv.stderr), sc.artifacts(host, case.mode, rh.returncode, rh.stdout, rh.stderr),
            rv, rh, av, ah)


_INPUT_LINES = {
    "--device-input": r"^\[input\] --device-input 1: (\d+) lines parsed on the device, (\d+) of them again on the host",
    "--device-bcf-input": r"^\[input\] --device-bcf-input 1: (\d+) records decoded on the device, (\d+) of them again on the host, [0-9.]+ GB of genotype bytes sent up; no fallback;",
    "--device-inflate": r"^\[input\] --device-inflate 1: (\d+) members inflated on the device, (\d+) compressed bytes sent up, (\d+) inflated bytes received, no fallback;",
}


def _input_stages_ran_on_the_device(case, stderr, where):
    for flag, pattern in _INPUT_LINES.items():
        if flag not in case.stages():
            continue
        m = re.search(pattern, stderr, re.M)
        assert m, (flag, "no [input] line without a fallback", [l for l in stderr.splitlines() if l.startswith("[input]")], where)
        if flag == "--device-inflate":
            assert int(m.group(1)) >= 1 and int(m.group(2)) > 0 and int(m.group(3)) > 0, (flag, m.group(0), where)
        else:                                                       # every record on the device, none handed back: they are inside the grammar
            assert (int(m.group(1)), int(m.group(2))) == (case.n_records, 0), (flag, m.group(0), case.n_records, where)


def _check(case, rng_mode, tmp, name):
    """run and compare; True when the case ran, False when both runs refused it with the same message"""
    dv, hv, rv, rh, av, ah = _pair(case, rng_mode, tmp, name)
    where = "\ndevice: %s\nhost:   %s\n" % (" ".join(av), " ".join(ah))
    if rv.returncode != 0:
        named = [f for f in list(sc.STAGES) + ["--records", "--devices", "--tile-sites"] if f in (dv["stderr"] or "")]
        assert not named, "a stage the table admits is refused: %s\n%s%s" % (named, dv["stderr"][-600:], where)
    skip = ("records",) if case.records0 else ()
    diff = sc.differences(dv, hv, skip=skip)
    assert not diff, "differs in %s; status %d / %d; %r%s" % (diff, rv.returncode, rh.returncode, {k: (str(dv[k])[-300:], str(hv[k])[-300:]) for k in diff
                                                                if k in ("stderr", "stdout", "discordance")}, where)
    if rv.returncode != 0:
        return False
    if case.records0:
        assert dv["records"] is None and hv["records"] is not None, where
    else:
        assert dv["records"] is not None, where
    _input_stages_ran_on_the_device(case, rv.stderr, where)
    return True


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_random_stage_runs_equal_their_host_twins(chunk, tmp_path):
    t0 = time.time()
    for k, case in enumerate(sc.fixed_cases(chunk, tmp_path, seed=SEED)):
        for rng_mode in (0, 1):
            ran = _check(case, rng_mode, tmp_path, "%d_%d" % (k, rng_mode))
            _seen["ran in --rng-mode %d" % rng_mode if ran else "refused by both in --rng-mode %d" % rng_mode] += 1
            if ran:
                side = tuple(f for f in ("--set-alleles", "--fetch-gl", "--gt-discordance") if case.has(f, None))
                _seen["stages: " + (" ".join(f[2:] for f in case.stages() + (("--records 0",) if case.records0 else ()) + side) or "none")] += 1
    _seen["seconds, chunk %d" % chunk] = round(time.time() - t0, 1)


def test_random_stage_runs_were_seldom_refused():
    """(runs after the chunks above) at most one configuration in ten may be one both paths refuse; prints what ran"""
    print("\nstage fuzz summary: " + json.dumps(_seen, sort_keys=True))
    ran = sum(v for k, v in _seen.items() if k.startswith("ran in"))
    refused = sum(v for k, v in _seen.items() if k.startswith("refused by both"))
    assert ran > 0 and 10 * refused <= ran + refused, dict(_seen)


def test_another_seed_is_a_difference_in_the_records(tmp_path):
    """negative control: the comparer sees that a device run with another --seed than its twin wrote other records"""
    case = sc.fixed_cases(0, tmp_path)[2]        # 35 records x 130 samples at depth 2, -O v: another seed draws other reads
    assert case.kind == "plain" and not case.records0 and case.n_sites >= 10 and case.has("--depth", "2.0"), case
    dv, hv, rv, rh, av, ah = _pair(case, 0, tmp_path, "same")
    assert rv.returncode == rh.returncode == 0 and sc.differences(dv, hv) == [], (av, ah)
    ref = list(case.ref_flags)
    ref[ref.index("--seed") + 1] = str((int(ref[ref.index("--seed") + 1]) + 1) % (2 ** 31 - 1))
    other = sc.dataclasses.replace(case, ref_flags=ref)
    out = str(tmp_path / "other")
    r = _run(other.argv(out, 0))
    ov = sc.artifacts(out, case.mode, r.returncode, r.stdout, r.stderr)
    assert r.returncode == 0 and "records" in sc.differences(ov, hv), (other.argv(out, 0), ah)
