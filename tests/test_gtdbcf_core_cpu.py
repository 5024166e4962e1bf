"""The rules of gtdiscordance_hip --bcf-direct 1 (vcfgl_amd/csrc/misc/gtdbcf_core.h: what the host path and k_gtd_bcf_decode run) on
the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/gtdbcf_core_main.cpp)
judges a corpus of typed vectors, each in a heap block of exactly its length -- every GT shape of tests/test_gtdisc_core_cpu.py that
numbers can say, at int8 / int16 / int32, one to three values a sample and the end-of-vector at every position; GQ at 0, 1, 127, 128,
missing, end-of-vector and negative; PL vectors for one to five alleles with too few and too many values, 9999, 10000 and negatives.
Required: what tests/gtdisc_model.py gives on the text a VCF writer makes of the same vectors (tests/gtdbcf_cases.py renders it as the
program's text route does), and no sanitizer report."""
import os
import re
import subprocess

import pytest

import gtdbcf_cases as gc
import gtdisc_model as gm
from test_gtdisc_core_cpu import ACGT, GTS, SIXTEEN, WITH_STAR, pl_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vcfgl_amd", "csrc")
M, E = gc.M, gc.E
LIMIT = {1: 127, 2: 32767, 3: 2 ** 31 - 1}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gtdbcf_core") / "gtdbcf_core_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "gtdbcf_core_main.cpp")]
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
    assert got[-1] == "" and len(got) == len(cases) + 1 and r.stdout.split()[:2] == ["cases", str(len(cases))]
    return got[:-1]


def fits(vals, t):
    return all(x in (M, E) or -LIMIT[t] + 1 < x <= LIMIT[t] for v in vals for x in v)


def vec(vals, t, n):
    """'TYPE N HEX' of the vectors (type 0: an absent field)"""
    if vals is None:
        return "0 0 -"
    return "%d %d %s" % (t, n, b"".join(gc.enc(x, t) for v in vals for x in v).hex() or "-")


def gt_shapes():
    """GT value lists (before padding): the token shapes of GTS that numbers can say, and the ones only numbers can"""
    out = []
    for tok in GTS:
        parts = re.split(r"[/|]", tok)
        seps = re.findall(r"[/|]", tok)
        if tok == "":
            out.append([])
        elif all(p == "." or (p.isdigit() and len(p) <= 3) for p in parts) and len(parts) <= 3:
            out.append([gc.gt_value(-1 if p == "." else int(p), int(k > 0 and seps[k - 1] == "|")) for k, p in enumerate(parts)])
    out += [[M, gc.gt_value(1)], [gc.gt_value(1), M], [M, M], [-3, gc.gt_value(0)], [gc.gt_value(0), -64], [0, 1], [gc.gt_value(99), gc.gt_value(99, 1)],
            [gc.gt_value(100), gc.gt_value(0)], [gc.gt_value(-1), gc.gt_value(17)], [gc.gt_value(-1), gc.gt_value(100)], [gc.gt_value(16383), gc.gt_value(0)],
            [2 ** 31 - 1, gc.gt_value(0)], [gc.gt_value(0), gc.gt_value(1), gc.gt_value(2)], [gc.gt_value(0), gc.gt_value(1), M]]
    return out


def padded(vals):
    """the list at 1, 2 and 3 values a sample (end-of-vector behind it), and with an end-of-vector put in at every position"""
    out = []
    for n in (1, 2, 3):
        if len(vals) <= n:
            out.append(vals + [E] * (n - len(vals)))
        for at in range(n):
            v = (vals + [gc.gt_value(1)] * 3)[:n]
            v[at] = E
            out.append(v)
    return out


def test_the_vector_corpus_in_blocks_of_exactly_their_length(program, tmp_path):
    cases, want = [], []
    NEIGHBOUR = {1: [gc.gt_value(3)], 2: [gc.gt_value(3), gc.gt_value(3)], 3: [gc.gt_value(3), gc.gt_value(3), gc.gt_value(3)]}

    def text_of(fields):
        return gc.columns(gc.Rec(1, ["A"], fields), 3)

    def true_case(v, t, nal, amap):
        gt = [NEIGHBOUR[len(v)], v, NEIGHBOUR[len(v)]]
        fmt, cols = text_of([("GT", t, len(v), gt)])
        cases.append("T 3 1 %d %x %s" % (nal, amap, vec(gt, t, len(v))))
        r = gm.plain_true(cols[1], 0, nal, amap)
        want.append("host" if r is None else "ok %d" % r)

    def call_case(v, t, nal, amap, mode, gq=None, gq_t=1, pl=None, pl_t=2):
        gt = [NEIGHBOUR[len(v)], v, NEIGHBOUR[len(v)]]
        fields = [("GT", t, len(v), gt)]
        gqv = plv = None
        if gq is not None:
            gqv = [[55] * len(gq), gq, [66] * len(gq)]
            fields.append(("GQ", gq_t, len(gq), gqv))
        if pl is not None:
            plv = [[0] * len(pl), pl, [0] * len(pl)]
            fields.append(("PL", pl_t, len(pl), plv))
        fmt, cols = text_of(fields)
        keys = fmt.split(":")
        cases.append("C 3 1 %d %d %x %s %s %s" % (mode, nal, amap, vec(gt, t, len(v)), vec(gqv, gq_t, len(gq or [])), vec(plv, pl_t, len(pl or []))))
        r = gm.plain_call(cols[1], 0, keys.index("GQ") if "GQ" in keys else -1, keys.index("PL") if "PL" in keys else -1, nal, amap, mode)
        want.append("host" if r is None else "ok %d %d" % r)

    for shape in gt_shapes():
        for v in padded(shape):
            for t in (1, 2, 3):
                if not fits([v], t):
                    continue
                for nal, amap in ((4, ACGT), (2, ACGT), (4, WITH_STAR), (16, SIXTEEN), (17, SIXTEEN)):
                    true_case(v, t, nal, amap)
                    call_case(v, t, nal, amap, gm.GQ_NONE)
                    call_case(v, t, nal, amap, gm.GQ_MAX)
    for gt in ([gc.gt_value(0), gc.gt_value(1)], [gc.gt_value(-1), gc.gt_value(-1)], [gc.gt_value(1), gc.gt_value(1, 1)], [gc.gt_value(2), gc.gt_value(0)],
               [gc.gt_value(0), gc.gt_value(3)], [gc.gt_value(0)]):
        for gq in ([0], [1], [9], [127], [128], [M], [E], [-1], [-5], [1000], [30, 7], [E, 30], [M, 30], []):
            for gq_t in (1, 2, 3):
                if not fits([gq], gq_t):
                    continue
                call_case(gt, 1, 3, ACGT, gm.GQ_TAG, gq=gq, gq_t=gq_t)
                call_case(gt, 2, 3, ACGT, gm.GQ_TAG, gq=gq, gq_t=gq_t, pl=[0, 1, 2, 3, 4, 5], pl_t=1)
    for nal in (1, 2, 3, 4, 5):
        nG = nal * (nal + 1) // 2
        for text in pl_vectors(nal):
            if not all(re.fullmatch(r"\.|-?[0-9]+", x) for x in text.split(",")):
                continue                                                # (an empty token: numbers cannot say it)
            vals = [M if x == "." else int(x) for x in text.split(",")]
            for pl in (vals, vals + [E], vals + [E, 0], [E] + vals):
                for pl_t in (1, 2, 3):
                    if not fits([pl], pl_t):
                        continue
                    for gt in ([gc.gt_value(0), gc.gt_value(0)], [gc.gt_value(-1), gc.gt_value(-1)], [gc.gt_value(0), gc.gt_value(nal - 1)], [gc.gt_value(0), gc.gt_value(nal)]):
                        amap = ACGT if nal < 5 else 0xFFFFFFFFFFF03210
                        call_case(gt, 1, nal, amap, gm.GQ_PL, pl=pl, pl_t=pl_t)
                        call_case(gt, 1, nal, amap, gm.GQ_PL, gq=[44], pl=pl, pl_t=pl_t)
    assert len(cases) > 10000
    got = run(program, tmp_path, cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])
    # the corpus reaches what it is meant to: both outcomes, missing calls, the GQ edges and the PL rule's branches
    assert "host" in want and "ok 255 0" in want and {"ok 16 1", "ok 16 127"} <= set(want)
    assert {int(w.split()[2]) for w in want if w.startswith("ok") and len(w.split()) == 3} >= {0, 1, 4, 7, 126, 127}
    assert want.count("host") > 1000 and sum(w.startswith("ok") for w in want) > 1000


def test_a_side_in_one_block_and_descriptors_that_do_not_fit(program, tmp_path):
    """gtd::bcf_side_plain over N samples of one block of exactly the vectors' bytes: the planes of a plain side; ST_HOST, and no read,
    for every descriptor that claims a byte more than the block has, a negative offset, an unknown type or a missing GT"""
    n = 5
    gt = [[gc.gt_value(a), gc.gt_value(b, 1)] for a, b in ((0, 1), (2, 2), (-1, 0), (3, 0), (1, 1))]
    gq = [[7], [127], [M], [1], [99]]
    blob = b"".join(gc.enc(x, 1) for v in gt for x in v) + b"".join(gc.enc(x, 2) for v in gq for x in v)
    cases, want = [], []

    def side(call, n_bytes, gt_d, gq_d, w):
        cases.append("S %d %d %d 4 %x %d %d %d %d %d %d %d 0 0 0 %s" % (call, n, gm.GQ_TAG if call else gm.GQ_NONE, ACGT, n_bytes, *gt_d, *gq_d, blob.hex()))
        want.append(w)

    bases = [(a if a >= 0 else 0) | ((b if b >= 0 else 0) << 4) for a, b in ((0, 1), (2, 2), (-1, 0), (3, 0), (1, 1))]
    cb = bytes(0xFF if k == 2 else x for k, x in enumerate(bases))
    ok_call = "ok %s %s" % (cb.hex(), bytes([7, 127, 0, 1, 99]).hex())
    side(1, len(blob), (0, 1, 2), (10, 2, 1), ok_call)
    side(0, len(blob), (0, 1, 2), (0, 0, 0), "host")                    # a truth side: sample 2 has a missing allele
    side(0, 4, (0, 1, 2), (0, 0, 0), "host")                            # ... and told of 4 bytes it reads none
    for n_bytes, gt_d, gq_d in ((len(blob) - 1, (0, 1, 2), (10, 2, 1)), (len(blob), (1, 1, 2), (11, 2, 1)), (len(blob), (0, 1, 2), (12, 2, 1)),
                                (len(blob), (-1, 1, 2), (10, 2, 1)), (len(blob), (0, 4, 2), (10, 2, 1)), (len(blob), (0, 1, 2), (10, 5, 1)),
                                (len(blob), (0, 2, 3), (10, 2, 1)), (len(blob), (0, 1, 2 ** 31 - 1), (10, 2, 1)), (len(blob), (0, 1, 2), (10, 3, 2 ** 31 - 1)),
                                (9, (0, 1, 2), (10, 2, 1)), (len(blob), (0, 1, 2), (0, 0, 0))):
        side(1, n_bytes, gt_d, gq_d, "host")
    got = run(program, tmp_path, cases)
    assert got == want
