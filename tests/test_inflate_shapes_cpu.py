"""Deflate streams that zlib's compressor never writes (tests/inflate_shapes.py, written by tests/deflate_builder.py) through the
inflater's decoder on the CPU: tests/inflate_core_main.cpp around vcfgl_amd/csrc/vgl_inflate_core.h, built and run under
AddressSanitizer and UndefinedBehaviorSanitizer as in test_inflate_core_cpu.py.  Every good member must come back OK with the
bytes that the builder's own expansion and zlib agree on, every refused one HOST by the check it was made for, every one-bit
mutant with zlib's verdict -- and the builder and the cases check themselves before any decoder sees them."""
import random
import zlib

import pytest

import deflate_builder as db
import inflate_corpus as ic
import inflate_shapes as sh
import test_inflate_core_cpu as tic

program, decode = tic.program, tic.decode


# ---- without the decoder

def test_the_builder_against_zlib_and_itself():
    rng = random.Random(1)
    for n, L in [(2, 1), (3, 2), (16, 15), (286, 15), (286, 9), (19, 7), (8, 7), (30, 15), (30, 5), (512, 9), (4, 2)]:
        lens = db.random_lengths(n, L, rng)
        assert db.kraft(lens) == 32768 and max(lens) == L and min(lens) >= 1 and len(lens) == n
        codes = db.canonical(lens)
        words = sorted(format(c, "0%db" % l) for c, l in codes.values())
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]))              # prefix-free
    assert [db.len_symbol(l)[0] for l in (3, 10, 11, 12, 257, 258)] == [257, 264, 265, 265, 284, 285] and db.len_symbol(258, True) == (284, 31, 5)
    assert [db.dist_symbol(d) for d in (1, 4, 5, 6, 24577, 32768)] == [(0, 0, 0), (3, 0, 0), (4, 0, 1), (4, 1, 1), (29, 0, 13), (29, 8191, 13)]
    assert db._rle([0] * 150 + [6] * 8 + [0] * 3 + [5, 5, 0]) == [(18, 127, 138), (18, 1, 12), (6, 0, 1), (16, 3, 6), (6, 0, 1), (17, 0, 3), (5, 0, 1), (5, 0, 1),
                                                                  (0, 0, 1)]
    # a stored, a fixed and a dynamic block of the same bytes against zlib; what zlib's own compressor wrote expands the same way
    text = ic.vcf_text(700, samples=20)
    toks = list(text[:300]) + [(40, 300), (258, 1), (3, 339)]
    want = bytearray(text[:300])
    for ln, d in toks[300:]:
        for _ in range(ln):
            want.append(want[-d])
    for blocks in ([db.stored(bytes(want))], [db.fixed(toks)], [db.dynamic(toks, seed=5)], [db.dynamic(toks, full=True, form="plain", hclen=19, seed=6)]):
        dfl, data = db.build(blocks)
        assert data == bytes(want) and db.check(dfl, data)
    # check() refuses what the issue's trial tripped over: bytes left over behind the final block, and a stream without a final block
    dfl, data = db.build([db.fixed(toks)])
    with pytest.raises(AssertionError):
        db.check(dfl + b"\0", data)
    with pytest.raises(AssertionError):
        db.check(db.build([db.fixed(toks, final=False)], raw=True)[0], data)
    with pytest.raises(AssertionError):
        db.check(dfl, data[:-1] + b"x")
    with pytest.raises(AssertionError):                                                  # not raw: an incomplete code is the builder's error
        db.build([db.dynamic([65], ll_lens={65: 2, 256: 2})])
    with pytest.raises(AssertionError):
        db.build([db.fixed([65, (3, 2)])])


def test_the_cases_assert_their_properties_and_zlib_agrees():
    good, bad = sh.shaped(), sh.refused()                 # (their own assertions run inside)
    names = {n for n, _, _ in good}
    assert {"ll_every_length_1_to_15", "d_every_length_1_to_15", "ll_longest_10", "ll_longest_11", "d_longest_9", "d_longest_10", "200_blocks",
            "stored_blocks_after_huffman_blocks_ending_at_every_bit_offset", "htslib_member_of_test10_pileup_gz"} <= names
    assert sum(1 for n in names if n.startswith("large_64_pairs_of_48_bits_at_phase_")) == 8
    assert sum(1 for n in names if n.startswith("large_48_bit_pair_then_15_bit_end_of_block_")) == 8
    assert {"isize_%d" % n for n in sh.SIZE_EDGES if n <= 4096} | {"large_isize_65535", "large_isize_65536"} <= names
    lens = sorted(sh.staging_in_lens().values())
    assert lens == list(sh.STAGING_LENS) and lens[0] < 8192 < lens[-1] and 8192 in lens and {n % 4 for n in lens if n > 8192} == {0, 1, 2, 3}
    for name, m, data in good:
        assert db.check(ic.deflate_of(m), data) and zlib.decompress(m, 31) == data, name
    assert len(good) >= 90 and len(bad) >= 29
    assert {c for _, _, c in bad} >= {7, 8, 10, 11, 12, 13, 14, 16, 18}               # the checks no test named before


def test_no_stream_is_dropped_and_both_verdicts_occur():
    streams, mutants = sh.fuzzed()
    assert (len(streams), len(mutants)) == sh.FUZZ[1:] == (500, 2000)
    accepted, refused = sh.mutant_counts()
    print("mutants accepted by zlib: %d, refused: %d" % (accepted, refused))
    assert accepted >= 100 and refused >= 100
    for name, m, data in streams:
        assert db.check(ic.deflate_of(m), data) and len(data) <= 4096, name
    kinds = {ic.deflate_of(m)[0] >> 1 & 3 for _, m, _ in streams}
    assert kinds == {0, 1, 2}


# ---- with the decoder under the sanitizers

def test_every_shaped_member_is_decoded(program, tmp_path):
    good = sh.shaped()
    got, stdout = decode(program, [m for _, m, _ in good], tmp_path)
    for (name, m, data), (status, check, out) in zip(good, got):
        assert (status, check) == (0, 0), (name, status, check)
        assert out == data, name
    assert "index 0 %d " % len(good) in stdout


def test_every_refused_member_is_refused_by_its_check(program, tmp_path):
    bad = sh.refused()
    got, stdout = decode(program, [m for _, m, _ in bad], tmp_path)
    wrong = [(name, want, (status, check)) for (name, _, want), (status, check, out) in zip(bad, got) if (status, check) != (1, want) or out != b""]
    assert wrong == []
    assert "index 0 %d " % len(bad) in stdout                          # the container of every one is whole


def test_every_fuzzed_stream_and_every_mutant_has_zlibs_verdict(program, tmp_path):
    streams, mutants = sh.fuzzed()
    got, _ = decode(program, [m for _, m, _ in streams] + [m for _, m, _ in mutants], tmp_path)
    for (name, m, data), (status, check, out) in zip(streams, got):
        assert (status, check) == (0, 0) and out == data, (name, status, check)
    wrong = []
    for (name, m, want), (status, check, out) in zip(mutants, got[len(streams):]):
        if want is None:
            if status != 1 or out != b"":
                wrong.append((name, "zlib refuses it", status, check))
        elif (status, check) != (0, 0) or out != want:
            wrong.append((name, "zlib accepts it", status, check))
    assert wrong == []
