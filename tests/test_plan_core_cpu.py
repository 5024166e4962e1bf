"""The launch plan (vcfgl_amd/csrc/hostlib/plan.h: argument validation and every derivation of vgl_ctx_create, a pure function) on
the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/plan_core_main.cpp,
no hooks) runs vgl_plan over the cases of tests/ctx_plan_cases.py and prints the fields of vgl_ctx_info that the plan decides --
through vgl_plan_info, the derivation vgl_ctx_info itself uses.  Required: what tests/golden/ctx_plan/parent_info.json records for
the library on a GPU (every field except workspace_bytes, device and test_hooks; the refusals' codes and texts), and no sanitizer
report.  The null-pointer case is vgl_ctx_create's own check, ahead of the plan, and stays with tests/test_gpu_ctx_plan.py."""
import json
import os
import subprocess

import pytest

import ctx_plan_cases as cpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctx_plan", "parent_info.json")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_core") / "plan_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "plan_core_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_the_plan_on_the_cpu_is_the_recorded_plan(program, tmp_path):
    cases = [c for c in cpc.CASES if not c.get("null")]
    path = tmp_path / "cases.txt"
    path.write_text("".join(cpc.case_line(c) + "\n" for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    lines = r.stdout.splitlines()
    assert [ln.split(" ", 1)[0] for ln in lines] == [c["name"] for c in cases]
    refused = 0
    for ln, case in zip(lines, cases):
        name, rest = ln.split(" ", 1)
        want = golden[name]
        if "code" in want:
            code, text = rest.split(" ", 1)
            assert code == f"code={want['code']}" and text == "error=" + want["error"], name
            refused += 1
            continue
        got = {k: int(v) for k, v in (w.split("=") for w in rest.split())}
        assert got == {k: v for k, v in want["info"].items() if k not in cpc.NOT_PLAN_FIELDS}, name
        if "info_after_tile" in want:                                   # a tile changes nothing the plan decides
            assert got == {k: v for k, v in want["info_after_tile"].items() if k not in cpc.NOT_PLAN_FIELDS}, name
    assert refused == sum(1 for c in cases if c["name"].startswith("refuse_")) >= 20
