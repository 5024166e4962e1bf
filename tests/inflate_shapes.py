"""BGZF members that no compressor in the tree writes, made by tests/deflate_builder.py from explicit descriptions, for the
inflater's tests (test_inflate_shapes_cpu.py, test_gpu_inflate_shapes.py):

    shaped()                         [(name, member bytes, the bytes it inflates to)]   good members, one property of RFC 1951 each
    refused()                        [(name, member bytes, check)]   whole BGZF members an inflater must refuse, with the number of
                                     the check of vgl_inflate_core that each was made for
    fuzzed(seed_base, n_streams, n_mutants)
                                     (streams, mutants): random valid members as in shaped(), and members with one flipped bit in
                                     the deflate part as (name, member bytes, zlib's bytes or None): zlib is the verdict

Every case asserts here, without any decoder under test, the property it is named for; every good stream went through
deflate_builder.check (zlib reaches the exact end and gives the builder's own expansion).  Outputs are a few hundred bytes to 4 KiB;
cases whose property needs more are named large_*, the staging cases (about 8 KiB) staging_*."""
import functools
import os
import random
import struct
import zlib

import deflate_builder as db
import inflate_corpus as ic

HERE = os.path.dirname(os.path.abspath(__file__))
CHAIN = list(range(1, 15)) + [15, 15]                    # 16 lengths, Kraft sum 1, every length 1 .. 15
OVERLAP_LENS = (3, 4, 63, 64, 65, 128, 257, 258)
SIZE_EDGES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536)
STAGING_LENS = (8191, 8192, 8193, 8194, 8195, 8196)      # both sides of the kernel's IN_LDS; beyond it every in_len mod 4
FUZZ = (20261, 500, 2000)                                # seed base, streams, mutants


class Toks:
    """tokens of one member as they are laid down, with the output position they have reached"""

    def __init__(self, seed):
        self.rng, self.t, self.n = random.Random(seed), [], 0

    def lit(self, v=None, alphabet=None):
        self.t.append(self.rng.randrange(256) if v is None and alphabet is None else self.rng.choice(alphabet) if v is None else v)
        self.n += 1

    def lits(self, k, alphabet=None):
        for _ in range(k):
            self.lit(alphabet=alphabet)

    def match(self, length, dist, alt=False):
        assert 1 <= dist <= self.n, (dist, self.n)
        self.t.append((length, dist, True) if alt else (length, dist)); self.n += length

    def skip(self, k):                                   # bytes another block (a stored one) produced
        self.n += k

    def fill(self, target):
        """up to `target` bytes of output that repeats at no fixed period, from few tokens: 512 random literals, then matches at
        random distances with a random literal behind each"""
        while self.n < target:
            rem = target - self.n
            if self.n < 512 or rem < 4:
                self.lit()
            else:
                self.match(self.rng.randint(3, min(258, rem - 1)), self.rng.randint(1, min(self.n, 32768)))
                self.lit()
        assert self.n == target

    def take(self):
        t, self.t = self.t, []
        return t


def _ll_used(tokens):
    return db._token_symbols(tokens)[0]


def _d_used(tokens):
    return db._token_symbols(tokens)[1]


@functools.lru_cache(maxsize=None)
def shaped():
    out = []

    def add(name, blocks):
        info = []
        m, data = db.member(blocks, info=info)
        out.append((name, m, data))
        return info

    # ---- codeword lengths
    lits15 = list(range(65, 80))
    ll_chain = dict(zip(lits15 + [256], CHAIN))          # 'A' one bit .. 'O' and the end-of-block code 15 bits
    t = Toks(1); [t.lit(v) for v in lits15]; t.lits(400, alphabet=lits15)
    toks = t.take()
    info = add("ll_every_length_1_to_15", [db.dynamic(toks, ll_lens=ll_chain)])
    assert {info[0]["ll_lens"][s] for s in _ll_used(toks)} == set(range(1, 16))
    for L in (10, 11):                                   # the direct table's edge: VGL_INF_FAST_LL bits and one more
        t = Toks(10 + L)
        for v in t.rng.sample(range(256), 256):
            t.lit(v)
        for s in range(29):
            t.match(db.LEN_BASE[s], t.rng.randint(1, 200))
        toks = t.take()
        info = add("ll_longest_%d" % L, [db.dynamic(toks, ll_max=L, seed=L)])
        assert len(_ll_used(toks)) == 285 and max(info[0]["ll_lens"]) == L == max(info[0]["ll_lens"][s] for s in _ll_used(toks))
    d_chain = dict(zip(range(16), CHAIN))

    def d16(seed):
        t = Toks(seed); t.lits(400)
        for k in range(48):
            s = k % 16
            t.match(t.rng.randint(3, 12), db.DIST_BASE[s] + t.rng.randrange(1 << db.dist_extra(s)))
        return t.take()
    toks = d16(2)
    info = add("d_every_length_1_to_15", [db.dynamic(toks, d_lens=d_chain)])
    assert {info[0]["d_lens"][s] for s in _d_used(toks)} == set(range(1, 16))
    for L in (9, 10):                                    # VGL_INF_FAST_D bits and one more
        toks = d16(20 + L)
        info = add("d_longest_%d" % L, [db.dynamic(toks, d_max=L, seed=L)])
        assert len(_d_used(toks)) == 16 and max(info[0]["d_lens"]) == L == max(info[0]["d_lens"][s] for s in _d_used(toks))
    t = Toks(3); t.lits(300, alphabet=lits15)
    info = add("cl_code_with_7_bit_codewords", [db.dynamic(t.take(), ll_lens=ll_chain, cl_max=7, form="plain", seed=3)])
    used_cl = {c[0] for c in info[0]["cl_syms"]}
    assert len(used_cl) >= 8 and max(info[0]["cl_lens"][s] for s in used_cl) == 7

    # ---- alphabets
    t = Toks(4)
    for v in t.rng.sample(range(256), 256):
        t.lit(v)
    t.fill(32768)
    for k in range(30):
        t.match(db.LEN_BASE[k % 29] + t.rng.randrange(1 << db.LEN_EXTRA[k % 29]), db.DIST_BASE[k] + t.rng.randrange(1 << db.dist_extra(k)))
    toks = t.take()
    assert _ll_used(toks) | {256} == set(range(286)) and _d_used(toks) == set(range(30))
    add("large_all_286_and_all_30_symbols_in_one_block", [db.dynamic(toks, full=True, seed=4)])
    t = Toks(5); t.lits(300)
    for L in range(3, 259):
        t.match(L, t.rng.randint(1, t.n))
    toks = t.take()
    assert {x[0] for x in toks if not isinstance(x, int)} == set(range(3, 259))
    add("large_every_length_3_to_258", [db.dynamic(toks, seed=5)])
    t = Toks(6); t.fill(32768)
    for s in range(30):
        for extra in (0, (1 << db.dist_extra(s)) - 1):
            t.match(t.rng.randint(3, 9), db.DIST_BASE[s] + extra)
    toks = t.take()
    dists = [x[1] for x in toks[-120:] if not isinstance(x, int)]
    assert 32768 in dists and 24577 in dists and all(db.DIST_BASE[s] in dists for s in range(30))
    add("large_every_distance_symbol_extra_bits_all_0_and_all_1", [db.dynamic(toks, seed=6)])
    t = Toks(7); t.lits(40); t.match(258, 5); t.match(258, 7, alt=True); t.lit(); t.match(258, 300, alt=True); t.match(258, 1)
    a = t.take()
    t.lits(9); t.match(258, 64, alt=True); t.match(258, 63)
    info = add("length_258_as_symbol_285_and_as_284_plus_31", [db.fixed(a), db.dynamic(t.take(), seed=7)])
    assert all(s in _ll_used(a) for s in (284, 285)) and info[1]["ll_lens"][284] and info[1]["ll_lens"][285]

    # ---- the longest pair: a 15-bit length code, 5 extra bits, a 15-bit distance code, 13 extra bits
    P, others = 112, list(range(97, 109))                # 'p' gets the one-bit code: k of them move the bit phase by k
    ll_run = dict(zip([P] + others + [256, 283, 284], CHAIN))
    ll_end = dict(zip([P] + others + [283, 284, 256], CHAIN))          # 284 and the end-of-block code 15 bits
    d_far = dict(zip(list(range(14)) + [28, 29], CHAIN))

    def pair(t):
        ln = t.rng.choice([195 + t.rng.randrange(32), 227 + t.rng.randrange(31)])
        t.match(ln, 16385 + t.rng.randrange(min(t.n, 32768) - 16384))
    phases = set()
    for phase in range(8):
        for k in range(8):                               # (the header is the same for every k: the first that gives the phase)
            t = Toks(30 + phase); t.fill(20000); hist = t.take()
            for _ in range(k):
                t.lit(P)
            for _ in range(64):
                pair(t)
            t.lits(3, alphabet=others)
            blocks, info = [db.fixed(hist), db.dynamic(t.take(), ll_lens=ll_run, d_lens=d_far)], []
            db.build(blocks, info=info)
            run = info[1]["tokens"][k:k + 64]
            if run[0][0] % 8 == phase:
                break
        assert len(run) == 64 and all(len(x) == 5 and x[4] - x[0] == 48 and (x[1] - x[0], x[2] - x[1], x[3] - x[2]) == (15, 5, 15) for x in run)
        assert all(x[0] % 8 == phase for x in run)
        phases.add(run[0][0] % 8)
        add("large_64_pairs_of_48_bits_at_phase_%d" % phase, blocks)
    assert phases == set(range(8))
    pads = set()
    for pad in range(8):
        for k in range(8):
            t = Toks(40 + pad); t.fill(17000); hist = t.take()
            for _ in range(k):
                t.lit(P)
            t.lits(5, alphabet=others)
            t.match(227 + t.rng.randrange(31), 16385 + t.rng.randrange(t.n - 16384))
            blocks, info = [db.fixed(hist), db.dynamic(t.take(), ll_lens=ll_end, d_lens=d_far)], []
            dfl, _ = db.build(blocks, info=info)
            if 8 * len(dfl) - info[1]["end"] == pad:
                break
        last, eob = info[1]["tokens"][-1], info[1]["eob"]
        assert last[4] - last[0] == 48 and eob == (last[4], last[4] + 15) and eob[1] == info[1]["end"] and 8 * len(dfl) - eob[1] == pad
        pads.add(pad)
        add("large_48_bit_pair_then_15_bit_end_of_block_%d_padding_bits" % pad, blocks)
    assert pads == set(range(8))                         # 0: the end-of-block code ends on bit 7 of the input's last byte

    # ---- overlapping copies: dist 1 .. 70, every dist with two lengths, 63 / 64 / 65 with all of them
    done = {}
    groups = [list(range(a, min(a + 5, 71))) for a in range(1, 71, 5)] + [[63], [64], [65]]
    for g, ds in enumerate(groups):
        t = Toks(50 + g)
        for d in ds:
            lens = OVERLAP_LENS if len(ds) == 1 else (OVERLAP_LENS[d % 8], OVERLAP_LENS[(d + 3) % 8])
            for ln in lens:
                t.lits(d)                                # the source: literals immediately before (the group's first at position dist)
                t.match(ln, d); done.setdefault(d, set()).add(ln)
        toks = t.take()
        assert isinstance(toks[ds[0] - 1], int) and toks[ds[0]][1] == ds[0]
        add("overlap_dist_%d_to_%d%s" % (ds[0], ds[-1], "_all_lengths" if len(ds) == 1 else ""),
            [db.fixed(toks) if g % 2 else db.dynamic(toks, seed=g)])
    assert set(done) == set(range(1, 71)) and all(len(v) >= 2 for v in done.values()) and all(done[d] == set(OVERLAP_LENS) for d in (63, 64, 65))
    t = Toks(70); t.lits(8)
    prev, n_chain = 8, 0
    for _ in range(40):                                  # each match begins inside the bytes the previous one wrote
        d = t.rng.randint(1, min(prev, 70)); ln = t.rng.choice([3, 5, 17, 63, 64, 65, 100])
        assert d <= prev
        t.match(ln, d); prev = ln; n_chain += 1
    assert n_chain >= 32
    add("chain_of_40_matches_each_from_the_previous_ones_tail", [db.dynamic(t.take(), seed=70)])
    t = Toks(71); payload = bytes(t.rng.randrange(256) for _ in range(200)); t.skip(200)
    t.match(100, 200); t.match(258, 64); t.match(65, 363); t.lit(); t.match(64, 65)
    a = t.take()
    payload2 = bytes(t.rng.randrange(256) for _ in range(70)); t.skip(70)
    t.match(128, 63); t.match(70, 70)
    add("matches_into_a_stored_blocks_bytes", [db.stored(payload), db.fixed(a), db.stored(payload2), db.dynamic(t.take(), seed=71)])
    t = Toks(72); t.lits(37); t.match(258, 37)
    assert t.t[-1] == (258, 37) and t.n - 258 == 37
    add("match_at_output_position_dist", [db.dynamic(t.take(), seed=72)])

    # ---- block sequences
    t, blocks = Toks(80), []

    def some_tokens(t, k):
        for _ in range(k):
            if t.n > 4 and t.rng.random() < 0.3:
                t.match(t.rng.randint(3, 20), t.rng.randint(1, min(t.n, 300)))
            else:
                t.lit(alphabet=b"ACGT\t01|\n")
        return t.take()
    for k in range(200):
        kind = t.rng.choice(["stored", "fixed", "dynamic"])
        if kind == "stored":
            p = bytes(t.rng.randrange(256) for _ in range(t.rng.randint(0, 20))); t.skip(len(p)); blocks.append(db.stored(p))
        elif kind == "fixed":
            blocks.append(db.fixed(some_tokens(t, t.rng.randint(0, 12))))
        else:
            blocks.append(db.dynamic(some_tokens(t, t.rng.randint(0, 12)), seed=k, form=t.rng.choice(["plain", "greedy", "cross"])))
    info = add("200_blocks", blocks)
    assert len(info) == 200 and {r["kind"] for r in info} == {"stored", "fixed", "dynamic"}
    for kind in ("stored", "fixed", "dynamic"):
        empty = {"stored": lambda: db.stored(b""), "fixed": lambda: db.fixed([]), "dynamic": lambda: db.dynamic([])}
        t = Toks(81); t.lits(50)
        blocks = [empty["dynamic"](), empty["fixed"](), empty["stored"](), db.fixed(t.take()), db.dynamic([], ll_max=3, d_max=2, seed=1),
                  empty["stored"](), empty["fixed"](), empty["dynamic"](), empty[kind]()]
        info = add("empty_blocks_then_a_final_empty_%s_block" % kind, blocks)
        assert info[-1]["final"] and info[-1]["kind"] == kind and not any(r["final"] for r in info[:-1])
    add("one_empty_final_dynamic_block", [db.dynamic([])])
    t, blocks = Toks(82), []
    for i in range(16):                                  # i nine-bit literals move the next stored block's header by i bits
        for _ in range(i):
            t.lit(200 + i)
        t.lit(65)
        blocks.append(db.fixed(t.take()))
        p = bytes(t.rng.randrange(256) for _ in range(5)); t.skip(5); blocks.append(db.stored(p))
    info = add("stored_blocks_after_huffman_blocks_ending_at_every_bit_offset", blocks)
    assert {r["start"] % 8 for r in info if r["kind"] == "stored"} == set(range(8))

    ll_long = dict(zip(lits15[1:] + [256] + list(range(257, 265)), CHAIN[1:] + [4] * 8))       # lengths 3 .. 10 at four bits, the rest 2 .. 15

    def block_long(t):                                   # 15-bit literal/length and distance codes
        t.lits(60, alphabet=lits15[1:])
        for k in range(16):
            t.match(t.rng.randint(3, 10), min(db.DIST_BASE[k], t.n))
        [t.lit(v) for v in lits15[1:]]
        return db.dynamic(t.take(), ll_lens=ll_long, d_lens=d_chain)

    def block_two_one_bit(t):                            # two one-bit codes and no distance code
        for _ in range(24):
            t.lit(66)
        return db.dynamic(t.take(), ll_lens={66: 1, 256: 1})

    def block_short_match(t):                            # a one-bit distance code behind tables of 15-bit codes
        t.lit(65); t.match(3, 1); t.lit(65); t.match(3, 1)
        return db.dynamic(t.take(), ll_lens={65: 2, 257: 2, 256: 1}, d_lens={0: 1})
    for name, order in (("15_bit_tables_then_two_one_bit_codes", "LTSL"), ("two_one_bit_codes_then_15_bit_tables", "TLSTL")):
        t = Toks(83); t.lits(400, alphabet=lits15)
        blocks = [db.fixed(t.take())] + [{"L": block_long, "T": block_two_one_bit, "S": block_short_match}[c](t) for c in order]
        info = add(name, blocks)
        longs = [r for r in info if r["kind"] == "dynamic" and max(r["ll_lens"]) == 15]
        assert longs and all(max(r["d_lens"]) == 15 for r in longs) and any(sorted(x for x in r["ll_lens"] if x) == [1, 1] for r in info[1:])
    t = Toks(84); t.lits(100); t.match(30, 50); a = t.take()
    t.lits(50); t.match(100, 170); b_ = t.take()
    p = bytes(t.rng.randrange(256) for _ in range(333)); t.skip(333)
    t.match(258, 333); t.lits(10)
    add("fixed_dynamic_stored_fixed", [db.fixed(a), db.dynamic(b_, seed=84), db.stored(p), db.fixed(t.take())])

    # ---- header forms
    def text_tokens(seed, k=300):
        t = Toks(seed)
        for _ in range(k):
            if t.n > 10 and t.rng.random() < 0.25:
                t.match(t.rng.randint(3, 40), t.rng.randint(1, t.n))
            else:
                t.lit(alphabet=b"ACGTNacgtn\t\n0123456789|./:")
        return t.take()
    for form in ("plain", "greedy"):
        info = add("header_form_%s" % form, [db.dynamic(text_tokens(90), form=form, seed=90)])
        assert (form == "plain") == all(c[0] < 16 for c in info[0]["cl_syms"])
    t = Toks(91); t.lits(200, alphabet=b"ACGT"); t.match(20, 40); t.match(30, 100)
    info = add("header_form_cross_a_run_from_the_literal_lengths_into_the_distance_lengths",
               [db.dynamic(t.take(), ll_lens={65: 2, 67: 3, 71: 3, 84: 3, 256: 3, 257 + 12: 3, 257 + 14: 3}, d_lens={10: 1, 13: 1}, hlit=280, form="cross")])
    at, crossing = 0, []
    for c in info[0]["cl_syms"]:
        if at < info[0]["hlit"] < at + c[2]:
            crossing.append(c)
        at += c[2]
    assert crossing and crossing[0][0] in (17, 18)
    six = {s: 6 for s in range(150, 182)}; six.update({256: 2, 257: 2})
    t = Toks(92); t.lits(300, alphabet=list(range(150, 182))); t.match(3, 7)
    info = add("header_form_maximal_runs_18_of_138_and_16s_of_6", [db.dynamic(t.take(), ll_lens=six, d_lens={5: 1}, hdist=30, form="maximal")])
    assert (18, 127, 138) in info[0]["cl_syms"]
    t = Toks(93); t.lits(200, alphabet=b"ACGT")
    info = add("hlit_257_hdist_1_hclen_minimal", [db.dynamic(t.take(), seed=93)])
    assert (info[0]["hlit"], info[0]["hdist"]) == (257, 1)
    info = add("hlit_286_hdist_30_hclen_19_padded_with_zero_lengths", [db.dynamic(text_tokens(94), hlit=286, hdist=30, hclen=19, seed=94)])
    assert (info[0]["hlit"], info[0]["hdist"], info[0]["hclen"]) == (286, 30, 19) and info[0]["ll_lens"][285] == 0 and info[0]["d_lens"][29] == 0
    assert info[0]["cl_lens"][db.CL_ORDER[18]] == 0
    info = add("hclen_19_plain_no_repeat_codes", [db.dynamic(text_tokens(95), hclen=19, form="plain", seed=95)])
    assert info[0]["hclen"] == 19
    t = Toks(96); t.lits(5); [t.match(t.rng.randint(3, 70), 1) for _ in range(6)]
    info = add("single_distance_code_of_one_bit_on_symbol_0", [db.dynamic(t.take(), seed=96)])
    assert info[0]["d_lens"] == [1]
    t = Toks(97); t.fill(25000); a = t.take()
    [t.match(t.rng.randint(3, 258), 24577 + t.rng.randrange(t.n - 24577)) for _ in range(12)]
    info = add("large_single_distance_code_of_one_bit_on_symbol_29", [db.fixed(a), db.dynamic(t.take(), seed=97)])
    assert info[1]["d_lens"] == [0] * 29 + [1] and info[1]["hdist"] == 30
    t = Toks(98); t.lits(300, alphabet=b"ACGT\n")
    info = add("no_distance_code_with_hdist_30", [db.dynamic(t.take(), hdist=30, seed=98)])
    assert info[0]["d_lens"] == [0] * 30
    info = add("a_run_ending_exactly_at_hlit_plus_hdist", [db.dynamic(text_tokens(99), hdist=30, form="cross", seed=99)])
    c = info[0]["cl_syms"]
    assert c[-1][0] in (17, 18) and sum(x[2] for x in c) == info[0]["hlit"] + info[0]["hdist"]

    # ---- the staging limit: a stored block sized to give the input length, then a short dynamic block with a match back into it
    for target in STAGING_LENS:
        t = Toks(100 + target)
        tail_len = len(db.build([db.stored(b"x" * 300), db.dynamic([65, (100, 250), 66], seed=1)])[0]) - 305
        n = target - 5 - tail_len
        p = bytes(t.rng.randrange(256) for _ in range(n)); t.skip(n)
        t.lit(65); t.match(100, 250); t.lit(66)
        blocks = [db.stored(p), db.dynamic(t.take(), seed=1)]
        assert len(db.build(blocks)[0]) == target
        add("staging_in_len_%d" % target, blocks)

    # ---- size edges of the write-out and of the CRC32 slices
    for n in SIZE_EDGES:
        t = Toks(200 + n)
        if n <= 4096:
            t.lits(n)
        else:
            t.fill(n)
        add(("large_" if n > 4096 else "") + "isize_%d" % n, [db.fixed(t.take())])

    # ---- the one member in the tree that htslib wrote, and the EOF member behind it
    raw = open(os.path.join(HERE, "golden", "ref_vcf", "reference", "test10", "test10.pileup.gz"), "rb").read()
    size = struct.unpack_from("<H", raw, 16)[0] + 1
    first, rest = raw[:size], raw[size:]
    data = zlib.decompress(first, 31)
    assert size == 132 and len(data) == 247 and ic.deflate_of(first)[0] & 7 == 5 and rest == ic.EOF
    db.check(ic.deflate_of(first), data)
    out.append(("htslib_member_of_test10_pileup_gz", first, data))
    out.append(("htslib_eof_member", rest, b""))

    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names)
    for name, m, data in out:
        db.check(ic.deflate_of(m), data)
        limit = 65536 if name.startswith("large_") else 9216 if name.startswith("staging_") else 4096
        assert len(data) <= limit and len(m) <= 65536, (name, len(data))
    return tuple(out)


def staging_in_lens():
    return {name: len(ic.deflate_of(m)) for name, m, _ in shaped() if name.startswith("staging_")}


@functools.lru_cache(maxsize=None)
def refused():
    out = []

    def add(name, check, blocks, cut=None, isize=None):
        """cut: the bit range (from the builder's positions) strictly inside which the data ends, at a byte boundary"""
        info = []
        dfl, data = db.build(blocks, raw=True, info=info)
        if cut is not None:
            lo, hi = cut(info)
            nb = [k for k in range(len(dfl) + 1) if lo < 8 * k < hi]
            assert nb, (name, lo, hi)
            dfl = dfl[:nb[0]]
        data = data if isize is None else data[:isize]
        out.append((name, ic.wrap(dfl, data), check))
    A, B = 65, 66
    lits = [A, B, A, A]
    # oversubscribed and incomplete code sets of the three alphabets
    add("oversubscribed_literal_length_code", 13, [db.dynamic(lits, ll_lens={A: 1, B: 1, 256: 1})])
    add("oversubscribed_distance_code", 14, [db.dynamic(lits + [(3, 1)], ll_lens={A: 2, B: 2, 257: 2, 256: 2}, d_lens={0: 1, 1: 1, 2: 1})])
    add("oversubscribed_code_length_code", 8, [db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, cl_lens={0: 1, 2: 1, 1: 1}, form="plain")])
    add("incomplete_literal_length_code", 13, [db.dynamic(lits, ll_lens={A: 2, B: 2, 256: 2})])
    add("incomplete_distance_code", 14, [db.dynamic(lits + [(3, 1)], ll_lens={A: 2, B: 2, 257: 2, 256: 2}, d_lens={0: 2, 1: 2})])
    add("incomplete_code_length_code", 8, [db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, cl_lens={0: 1, 2: 2}, form="plain")])
    # the header's length sequence
    blk = db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, cl_lens={16: 1, 0: 2, 2: 2})
    blk["cl_syms"] = [(16, 0, 3)] + [(0, 0, 1)] * 255
    add("repeat_code_16_first", 10, [blk])
    blk = db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, cl_lens={18: 1, 0: 2, 2: 2})
    blk["cl_syms"] = [(18, 127, 138), (18, 110, 121)]                 # 259 lengths where HLIT + HDIST is 258
    add("run_past_hlit_plus_hdist", 11, [blk])
    add("no_end_of_block_code", 12, [db.dynamic(lits, ll_lens={A: 1, B: 1}, eob=False)])
    for n in (287, 288):
        add("hlit_%d" % n, 7, [db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, hlit=n)])
    for n in (31, 32):
        add("hdist_%d" % n, 7, [db.dynamic(lits, ll_lens={A: 2, B: 2, 67: 2, 256: 2}, hdist=n)])
    # symbols outside the alphabets, and unused patterns
    for s in (286, 287):
        add("fixed_block_literal_length_symbol_%d" % s, 16, [db.fixed(lits + [("ll", s)])])
    for s in (30, 31):
        add("fixed_block_distance_symbol_%d" % s, 18, [db.fixed(lits + [("ll", 257), ("d", s)])])
    add("unused_pattern_of_a_one_bit_distance_code", 17, [db.dynamic(lits + [("ll", 257), ("bits", 1, 1)], ll_lens={A: 2, B: 2, 257: 2, 256: 2}, d_lens={0: 1})])
    add("unused_pattern_of_a_one_bit_literal_length_code", 15, [db.dynamic([("bits", 1, 1)], ll_lens={256: 1}, eob=False)])
    # a distance one beyond the bytes produced
    add("distance_1_at_position_0", 19, [db.fixed([(3, 1)])])
    add("distance_one_beyond_a_stored_block", 19, [db.stored(b"0123456789"), db.fixed([(3, 11)])])
    add("distance_one_beyond_a_match", 19, [db.fixed([A, (5, 1), (3, 7)])])
    add("match_running_past_isize", 5, [db.fixed([A, B, (10, 2)])], isize=8)
    # the input ends early: 2 where the bit reader reports it, 15 / 17 where the symbol decode does
    add("input_ends_inside_length_extra_bits", 2, [db.fixed([200, (140, 1)])], cut=lambda i: (i[0]["tokens"][1][1], i[0]["tokens"][1][2]))
    add("input_ends_inside_distance_extra_bits", 2, [db.fixed([200, (3, 20000)])], cut=lambda i: (i[0]["tokens"][1][3], i[0]["tokens"][1][4]))
    add("input_ends_inside_a_stored_header", 2, [db.fixed(lits, final=False), db.stored(b"abc")], cut=lambda i: (i[1]["start"] + 8, i[1]["start"] + 24))
    add("no_final_block_ever", 2, [db.fixed(lits, final=False), db.fixed(lits, final=False)])
    add("input_ends_inside_a_literal_length_codeword", 15, [db.fixed([A, 200, 200])], cut=lambda i: i[0]["tokens"][1])
    add("input_ends_inside_a_distance_codeword", 17, [db.fixed([200, 200, (3, 1), A])], cut=lambda i: (i[0]["tokens"][2][2], i[0]["tokens"][2][3]))
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names)
    for name, raw, check in out:
        assert raw[:4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", raw, 16)[0] + 1 == len(raw) <= 65536, name
        isize = struct.unpack_from("<I", raw, len(raw) - 4)[0]
        assert isize <= 65536, name
        try:                                             # zlib refuses every one of them as a gzip member
            ok = len(zlib.decompress(raw, 31)) == isize
        except zlib.error:
            ok = False
        assert not ok, name
    assert {c for _, _, c in out} >= {2, 5, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19}
    return tuple(out)


FORMS = ("plain", "greedy", "cross")


def random_blocks(rng, seed):
    """1 .. 6 blocks of random kind with random tokens, random complete code lengths with a random longest codeword and a random
    header form; at most 4 KiB of output"""
    t = Toks(seed)
    t.rng = rng
    blocks, budget = [], rng.choice([0, 1, 50, 300, 1500, 4096])
    for k in range(rng.randint(1, 6)):
        share = rng.randint(0, max(0, budget - t.n)) if budget > t.n else 0
        kind = rng.choice(["stored", "fixed", "dynamic"])
        if kind == "stored":
            p = bytes(rng.randrange(256) for _ in range(share)); t.skip(share); blocks.append(db.stored(p))
            continue
        end = t.n + share
        alphabet = [rng.randrange(256) for _ in range(rng.choice([1, 2, 4, 16, 64, 256]))]
        p_match = rng.choice([0.0, 0.1, 0.5])
        while t.n < end:
            if t.n > 0 and end - t.n >= 3 and rng.random() < p_match:
                t.match(rng.randint(3, min(258, end - t.n)), rng.randint(1, min(t.n, 32768) if rng.random() < 0.5 else min(t.n, 40)))
            else:
                t.lit(alphabet=alphabet)
        if kind == "fixed":
            blocks.append(db.fixed(t.take()))
        else:
            blocks.append(db.dynamic(t.take(), full=rng.random() < 0.15, hlit=rng.choice([None, None, 286]), hdist=rng.choice([None, None, 30]),
                                     hclen=rng.choice([None, None, 19]), form=rng.choice(FORMS), seed=rng.randrange(1 << 30)))
    return blocks


def zlib_verdict(deflate):
    """zlib's bytes when it takes the raw deflate data to its exact end within 65536 bytes of output, else None"""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(deflate, 65537)
    except zlib.error:
        return None
    if not d.eof or d.unused_data != b"" or d.unconsumed_tail != b"" or len(got) > 65536:
        return None
    return got


@functools.lru_cache(maxsize=None)
def fuzzed(seed_base=FUZZ[0], n_streams=FUZZ[1], n_mutants=FUZZ[2]):
    streams = []
    for k in range(n_streams):                           # none is dropped: a stream the builder and zlib disagree on is a builder bug
        m, data = db.member(random_blocks(random.Random(seed_base + k), seed_base + k))
        assert len(data) <= 4096
        streams.append(("stream_%d" % k, m, data))
    rng, mutants = random.Random(seed_base - 1), []
    for k in range(n_mutants):
        j = rng.randrange(n_streams)
        _, m, data = streams[j]
        dfl = bytearray(ic.deflate_of(m))
        bit = rng.randrange(8 * len(dfl))
        dfl[bit >> 3] ^= 1 << (bit & 7)
        got = zlib_verdict(bytes(dfl))
        # accepted: the trailer of zlib's bytes, and the decoder must give them; refused: the original trailer, and HOST
        mutants.append(("stream_%d_bit_%d" % (j, bit), ic.wrap(bytes(dfl), data if got is None else got), got))
    accepted = sum(1 for _, _, g in mutants if g is not None)
    if n_mutants >= 2000:                                # both verdicts often enough to mean something
        assert accepted >= 100 and n_mutants - accepted >= 100, (accepted, n_mutants - accepted)
    return tuple(streams), tuple(mutants)


def mutant_counts():
    _, mutants = fuzzed()
    accepted = sum(1 for _, _, g in mutants if g is not None)
    return accepted, len(mutants) - accepted


def lz_tokens(data):
    """the tokens of `data` from a plain greedy matcher over three-byte keys (the last position of each): text for the builder to
    write, owing nothing to a compressor's choices"""
    toks, last, i, n = [], {}, 0, len(data)
    while i < n:
        j = last.get(data[i:i + 3]) if i + 3 <= n else None
        if j is not None and i - j <= 32768:
            ln = 3
            while ln < 258 and i + ln < n and data[j + ln] == data[i + ln]:
                ln += 1
            toks.append((ln, i - j))
            for k in range(i, i + ln):
                last[data[k:k + 3]] = k
            i += ln
        else:
            toks.append(data[i]); last[data[i:i + 3]] = i; i += 1
    return toks


def bgzf_by_builder(data, seed=0):
    """(file bytes, members): `data` as BGZF in members of 1 .. 3 KiB of input, written by the builder in turn as a stored block, a
    fixed block, a dynamic block with 15-bit literal/length and distance codes, and several blocks of changing kind; the EOF member last"""
    rng, members, i, k = random.Random(seed), [], 0, 0
    while i < len(data):
        piece = data[i:i + rng.randint(1024, 3072)]
        toks, form = lz_tokens(piece), k % 4
        if form == 0:
            blocks = [db.stored(piece)]
        elif form == 1:
            blocks = [db.fixed(toks)]
        elif form == 2:
            blocks = [db.dynamic(toks, ll_max=15, d_max=15, seed=seed + k, form=FORMS[k // 4 % 3])]
        else:
            cuts = sorted(rng.sample(range(1, len(toks)), 4))
            parts = [toks[a:b] for a, b in zip([0] + cuts, cuts + [len(toks)])]
            blocks = [db.fixed(p) if q % 2 else db.dynamic(p, seed=seed + k + q, form=FORMS[q % 3], hclen=19 if q == 2 else None) for q, p in enumerate(parts)]
        m, got = db.member(blocks)
        assert got == piece
        members.append(m); i += len(piece); k += 1
    return b"".join(members) + ic.EOF, len(members) + 1


def vcf_for_the_host_program(lines=300, samples=50):
    text = ("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (lines + 1) +
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(samples)) + "\n").encode()
    rng = random.Random(9)
    rows = []
    for i in range(lines):
        rows.append("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t%s\n" % (i + 1, "\t".join(rng.choices(["0|0", "0|1", "1|0", "1|1"], [85, 6, 6, 3], k=samples))))
    return text + "".join(rows).encode()
