"""The rules of the resident split (vcfgl_amd/csrc/misc/rf_core.h: what the kernels of resident_file.hip run) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/rf_core_main.cpp), every text in a heap
block of exactly its length.  The host model of the four passes, at chunk sizes 1, 2, 16, 64 and RF_CHUNK, must give what the
program's own line walk (memchr, nine_columns) gives, and scan_text must read from the head stream what it reads from the text:
on a few thousand random texts over the alphabet "\\n\\t#:,.A1" and on the hand-written texts the GPU tests also use.
Required: `ok` for every case and no sanitizer report."""
import os
import subprocess

import pytest

import miscread_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rf_core") / "rf_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "rf_core_main.cpp"), "-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(program, tmp_path, cases):
    fin, fout = str(tmp_path / "cases.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write("".join(c + "\n" for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = open(fout).read().split("\n")
    assert got[-1] == "" and len(got) == len(cases) + 1 and r.stdout.split()[:3] == ["cases", str(len(cases)), "RF_CHUNK"]
    return got[:-1]


@pytest.fixture(scope="module")
def chunk(program, tmp_path_factory):
    """RF_CHUNK as the program prints it (a run without cases)"""
    d = tmp_path_factory.mktemp("rf_chunk_cpu")
    open(str(d / "none.txt"), "w").close()
    r = subprocess.run([program, str(d / "none.txt"), str(d / "out.txt")], capture_output=True, text=True, timeout=60)
    word = r.stdout.split()
    assert r.returncode == 0 and word[:2] == ["cases", "0"] and word[2] == "RF_CHUNK", r.stdout
    c = int(word[3])
    assert c >= 64 and c % 16 == 0
    return c


def test_random_texts(program, tmp_path):
    got = run(program, tmp_path, ["R %d 1000" % seed for seed in (1, 2, 3, 4)])
    assert all(g.startswith("ok ") for g in got), got
    lines, over, records = (sum(int(g.split()[k]) for g in got) for k in (1, 2, 3))
    assert lines > 20000 and over > 100 and records > 5000          # the draws reach record lines, and lines too long for head-most 7


def hand_written(C):
    """name -> (text, head_most): the boundary texts of tests/test_gpu_resident.py and a few of a line or two"""
    n = 3
    t = {}
    for place in ("newline", "tab9", "begin"):
        for k, off in (("last", 2 * C - 1), ("first", 2 * C)):
            if place == "begin" and k == "last":
                continue
            t["%s_%s" % (place, k)] = U.text_with(n, 4, place, off)
    t["three_chunks"] = U.text_with(n, 2, "newline", 4 * C + 17)      # the record's line begins in chunk 0 or 1 and ends in chunk 4
    for d in (-1, 0, 1):
        t["total_%+d" % d] = U.text_of_length(n, 2 * C + d)
    t["total_c_plus_minus"] = U.text_of_length(n, C + 1)
    t["no_trailing_newline"] = U.text_of_length(n, C + 300, newline=False)
    body = ("\n".join(U.HEAD + [U.names_line(n)]) + "\n").encode()
    recs = [U.record(10 + i, n).encode() for i in range(4)]
    t["empty_lines"] = b"\n\n" + body + b"\n" + recs[0] + b"\n\n\n" + recs[1] + b"\n" + recs[2] + b"\n\n\n"
    t["header_line_after_records"] = body + recs[0] + b"\n" + recs[1] + b"\n##late=1\n" + recs[2] + b"\n"
    t["header_only"] = body
    t["eight_columns"] = body + recs[0] + b"\n" + U.record(11, n, columns=8).encode() + b"\n" + recs[2] + b"\n"
    out = {k: (v, 1 << 20) for k, v in t.items()}
    out["head_most_64"] = (U.text_with(n, 2, "tab9", 700), 64)
    for k, v in (("empty", b""), ("one_newline", b"\n"), ("no_newline", b"A"), ("hash", b"#"), ("nine_tabs", b"\t" * 9), ("ten_tabs_nl", b"\t" * 10 + b"\n"),
                 ("tab9_at_end", b"a\tb\tc\td\te\tf\tg\th\ti\t"), ("tab9_then_nl", b"a\tb\tc\td\te\tf\tg\th\ti\t\nx")):
        out[k] = (v, 1 << 20)
        out[k + "_most_1"] = (v, 1)
    return out


def test_hand_written_texts(program, chunk, tmp_path):
    cases = hand_written(chunk)
    got = run(program, tmp_path, ["T %d %s" % (most, text.hex() or "-") for text, most in cases.values()])
    res = dict(zip(cases, got))
    assert all(g.startswith("ok ") for g in got), res
    assert res["head_most_64"].split()[2] == "1" and res["newline_last"].split()[2] == "0"      # `over` is raised there, and nowhere else among these
    assert res["header_only"].split()[1:] == ["4", "0", "0"] and res["eight_columns"].split()[3] == "3" and res["empty"] == "ok 0 0 0"
    assert res["empty_lines"].split()[1] == str(4 + 3 + 2 + 1 + 2 + 2) and res["no_trailing_newline"].split()[1] == "8"
