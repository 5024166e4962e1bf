"""The reference model of the device BGZF compressor (tests/bgzf_model.py) checked without a GPU: its members inflate with zlib
and pass the strict inflater, its codes cost what an optimal Huffman code costs, the chosen block is the smallest of the three,
tokens keep deflate's and the parse's limits, the corpus reaches every length and distance code at both ends of its extra
bits, and the built inputs drive the length limit's Kraft repair."""
import functools
import zlib

import pytest

import bgzf_model as bm


@functools.lru_cache(maxsize=None)
def _members():
    out = []
    for name, data in bm.corpus().items():
        for i in range(0, len(data), bm.MEMBER):
            out.append((name, i // bm.MEMBER, data[i:i + bm.MEMBER], bm.member(data[i:i + bm.MEMBER])))
    return out


def test_members_inflate_strictly():
    for name, k, piece, m in _members():
        assert zlib.decompress(m.deflate, -15) == piece, (name, k)
        r = bm.inflate_member(m.raw)
        assert r["out"] == piece and r["btype"] == m.mode, (name, k)
        if m.mode:
            want = [(piece[p],) if not l else (l, d) for p, l, d in m.tokens]
            assert r["tokens"] == want, (name, k)
        if m.mode == 2:
            assert r["len_ll"] == m.len_ll[:m.hlit] and r["len_d"] == m.len_d[:m.hdist] and r["len_cl"] == m.len_cl, (name, k)
            # HLIT, HDIST and HCLEN trimmed: the last length each sends is nonzero (or the count is at its minimum)
            assert r["hclen"] == m.hclen and (m.hclen == 4 or m.len_cl[bm.CL_ORDER[m.hclen - 1]]), (name, k)
            assert m.hlit == 257 or m.len_ll[m.hlit - 1], (name, k)
            assert m.hdist == 1 or m.len_d[m.hdist - 1], (name, k)


def test_small_members_inflate_strictly():
    for n in list(range(1, 40)) + [63, 64, 65, 511, 512, 513]:
        for piece in (bytes(n), bytes(range(256)) * (n // 256) + bytes(range(n % 256)), b"ab" * (n // 2) + b"a" * (n % 2)):
            m = bm.member(piece)
            assert bm.inflate_member(m.raw)["out"] == piece, n


def test_codes_cost_an_optimal_huffman_code():
    checked = 0
    for name, k, _, m in _members():
        for key, hist, lens, limit in (("ll", m.hist_ll, m.len_ll, 15), ("d", m.hist_d, m.len_d, 15), ("cl", m.cl_hist, m.len_cl, 7)):
            w = list(hist)
            for s in range(len(w)):                        # the two-code minimum, as the model completes it
                if sum(1 for x in w if x) >= 2:
                    break
                if not w[s]:
                    w[s] = 1
            cost = sum(f * l for f, l in zip(w, lens))
            if m.depth[key] <= limit:
                assert m.repair[key] == 0 and cost == bm.huffman_cost(w), (name, k, key)
                checked += 1
            else:
                assert m.repair[key] > 0 and cost > bm.huffman_cost(w), (name, k, key)
    assert checked > 30


def test_chosen_block_is_the_smallest():
    for name, k, piece, m in _members():
        sizes = {}
        for mode in (0, 1, 2):
            f = bm.member(piece, force_mode=mode)
            assert zlib.decompress(f.deflate, -15) == piece and bm.inflate(f.deflate)["btype"] == mode, (name, k, mode)
            sizes[mode] = len(f.deflate)
        assert len(m.deflate) == min(sizes.values()) == sizes[m.mode], (name, k, sizes, m.mode)
        assert m.raw == bm.member(piece, force_mode=m.mode).raw


def test_tokens_keep_the_limits():
    for name, k, piece, m in _members():
        pos = 0
        for p, l, d in m.tokens:
            assert p == pos
            if l:
                assert 3 <= l <= 258 and 1 <= d <= min(32768, p), (name, k, p, l, d)
                assert p // bm.SEG == (p + l - 1) // bm.SEG, (name, k, p, l)          # no match crosses a segment end
                assert piece[p - d:p - d + l] == piece[p:p + l] or all(piece[p + i] == piece[p - d + i] for i in range(l))
            pos = p + (l or 1)
        assert pos == len(piece)
        if m.seg_bits is not None:
            assert len(m.seg_bits) == -(-len(piece) // bm.SEG) and m.hdr_bits + sum(m.seg_bits) + (7 if m.mode == 1 else m.len_ll[256]) == m.bits[m.mode]


def test_corpus_reaches_every_code_at_both_ends():
    lens, dists = set(), set()
    for _, _, _, m in _members():
        for p, l, d in m.tokens:
            if l:
                lens.add(l)
                dists.add(d)
    need_l = {x for i, b in enumerate(bm.LEN_BASE) for x in (b, b + (1 << bm.LEN_EB[i]) - 1 - (i == 27))}    # (284 ends at 257)
    need_d = {x for i, b in enumerate(bm.DIST_BASE) for x in (b, b + (1 << bm.DIST_EB[i]) - 1)}
    assert len(need_l) == 2 * 29 - 9 and len(need_d) == 2 * 30 - 4             # (codes without extra bits have one end)
    assert need_l <= lens, sorted(need_l - lens)
    assert need_d <= dists, sorted(need_d - dists)
    assert {int(bm.LSYM[l]) for l in lens} == set(range(257, 286)) and {int(bm.DSYM[d]) for d in dists} == set(range(30))


def test_built_inputs_drive_the_kraft_repair():
    c = bm.corpus()
    d = bm.member(c["deep_dist"])
    assert d.depth["d"] > 15 and d.repair["d"] > 0 and max(d.len_d) == 15
    cl = bm.member(c["deep_cl"])
    assert cl.depth["cl"] > 7 and cl.repair["cl"] > 0 and max(cl.len_cl) == 7
    for m in (d, cl):
        r = bm.inflate_member(m.raw)                     # complete codes within the limits after the repair
        assert r["len_d"] == m.len_d[:m.hdist] and r["len_cl"] == m.len_cl
    print("deep_dist: distance depth %d, %d repair steps; deep_cl: code-length depth %d, %d repair steps"
          % (d.depth["d"], d.repair["d"], cl.depth["cl"], cl.repair["cl"]))


def test_build_lengths_against_heapq_on_random_histograms():
    import numpy as np
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(2, 287))
        f = (rng.geometric(0.3, n) * (rng.random(n) < 0.7)).tolist()
        if sum(1 for x in f if x) < 2:
            continue
        lens, depth, steps = bm.build_lengths(f, 15)
        assert sum(1 << (15 - l) for l in lens if l) == 1 << 15
        if depth <= 15:
            assert steps == 0 and sum(a * b for a, b in zip(f, lens)) == bm.huffman_cost(f)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tiny_members(n):
    piece = bytes(range(n))
    m = bm.member(piece)
    assert m.mode == 1 and zlib.decompress(m.deflate, -15) == piece


def test_lazy_rule_and_segment_end():
    # at the second "abc", "abc" (3 bytes, 10 back) loses to "bcdef" one byte on: a literal, then the longer match
    data = b"abcQbcdefRabcdefS"
    m = bm.member(data)
    assert [(l, d) for _, l, d in m.tokens if l] == [(5, 7)] and [data[p] for p, l, _ in m.tokens if not l].count(ord("a")) == 2
    # a match of 32 or more is taken even when the next position has a longer one
    body = bytes(range(40, 80))
    m = bm.member(b"x" + body[:34] + b"Q" + body[1:40] + b"R" + body)
    assert (76, 34, 75) in m.tokens
    # a repeat across position 512 ends at the segment's end and starts again there
    data = bytes(range(200)) + bytes(range(200)) * 3
    m = bm.member(data)
    assert all(p // bm.SEG == (p + l - 1) // bm.SEG for p, l, _ in m.tokens if l)
    assert any(p + l == bm.SEG for p, l, _ in m.tokens if l) and any(p == bm.SEG and l for p, l, _ in m.tokens)
