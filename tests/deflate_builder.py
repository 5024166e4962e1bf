"""Raw deflate data (RFC 1951) written from an explicit description, independent of any compressor: the test-suite's own encoder
for the inflater's tests (tests/inflate_shapes.py).  A member is a list of blocks:

    stored(payload)                          BTYPE 00, any length 0 .. 65535
    fixed(tokens)                            BTYPE 01
    dynamic(tokens, ...)                     BTYPE 10 with code lengths given per symbol or generated, and a chosen header form

A token is a literal (int 0 .. 255) or a match (length, distance); (258, distance, True) writes length 258 as symbol 284 with
extra bits 31 instead of symbol 285.  build(blocks) expands the tokens itself and returns (deflate bytes, expected output);
check(deflate, data) is the second, independent reference: zlib.decompressobj(-15) must reach `eof` with no `unused_data` and give
the builder's bytes.  With raw=True nothing is asserted about validity and three more tokens exist, for streams an inflater must
refuse: ("ll", symbol) and ("d", symbol) write one codeword alone, ("bits", value, count) writes bits as they are.

Generated code lengths are complete (Kraft sum exactly 1) with a chosen longest codeword, from a seeded random.Random; the alphabet
is the used symbols (and as many unused ones as the longest codeword needs), or all 286 / 30 with full=True.
Header forms (`form`): "plain" one code-length symbol per length; "greedy" runs as 16 / 17 / 18, literal/length and distance
lengths apart (what zlib's send_tree does); "cross" the same over the joined sequence, so that a run may cross from the
literal/length lengths into the distance lengths; "maximal" like "cross", and the builder asserts that an 18 of 138 and two
16s of 6 in a row were written.  hlit / hdist / hclen: None for the smallest the lengths allow, or a count up to 286 / 30 / 19."""
import random
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def dist_extra(s):
    return 0 if s < 4 else (s >> 1) - 1


def len_symbol(length, alt258=False):
    """(symbol, extra value, extra bits) of a match length"""
    assert 3 <= length <= 258, length
    if length == 258:
        return (284, 31, 5) if alt258 else (285, 0, 0)
    assert not alt258
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    assert length - LEN_BASE[s] < 1 << LEN_EXTRA[s]
    return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]


def dist_symbol(d):
    assert 1 <= d <= 32768, d
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    assert d - DIST_BASE[s] < 1 << dist_extra(s)
    return s, d - DIST_BASE[s], dist_extra(s)


class Bits:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    @property
    def nbits(self):
        return 8 * len(self.buf) + self.n

    def put(self, v, k):                       # LSB first: header fields, extra bits
        assert 0 <= v < 1 << k, (v, k)
        self.acc |= v << self.n; self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, c, k):                      # a Huffman codeword: most significant bit first
        self.put(int(format(c & ((1 << k) - 1), "0%db" % k)[::-1], 2), k)      # (masked: an oversubscribed code of a raw case)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def kraft(lens):
    """the Kraft sum of the nonzero lengths, in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def canonical(lens):
    """{symbol: (codeword, length)} of the canonical code (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0], code, nxt = 0, 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1; nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


def random_lengths(n, longest, rng):
    """n code lengths with Kraft sum exactly 1 and the longest exactly `longest`: the chain 1, 2, .., longest, longest, then random
    leaves shorter than `longest` split in two until there are n"""
    assert 1 <= longest <= 15 and longest + 1 <= n <= 1 << longest, (n, longest)
    ls = list(range(1, longest)) + [longest, longest]
    while len(ls) < n:
        i = rng.choice([i for i, l in enumerate(ls) if l < longest])
        ls[i] += 1; ls.append(ls[i])
    rng.shuffle(ls)
    assert kraft(ls) == 32768 and max(ls) == longest and len(ls) == n
    return ls


def stored(payload, final=None):
    return dict(kind="stored", payload=bytes(payload), final=final)


def fixed(tokens, final=None, eob=True):
    return dict(kind="fixed", tokens=list(tokens), final=final, eob=eob)


def dynamic(tokens, ll_lens=None, d_lens=None, cl_lens=None, ll_max=None, d_max=None, cl_max=None, full=False, hlit=None, hdist=None,
            hclen=None, form="greedy", seed=0, final=None, eob=True):
    """ll_lens / d_lens / cl_lens: {symbol: length} or a list, or None for generated lengths with the longest codeword ll_max /
    d_max / cl_max (None: drawn from what the alphabet allows)"""
    return dict(kind="dynamic", tokens=list(tokens), ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens, ll_max=ll_max, d_max=d_max, cl_max=cl_max,
                full=full, hlit=hlit, hdist=hdist, hclen=hclen, form=form, seed=seed, final=final, eob=eob)


def _as_list(lens, n):
    if isinstance(lens, dict):
        out = [0] * n
        for s, l in lens.items():
            out[s] = l
        return out
    return list(lens) + [0] * (n - len(lens))


def _generate(used, size, longest, full, rng, cap=15):
    """lengths of an alphabet of `size` symbols that holds `used`"""
    syms = set(range(size)) if full else set(used)
    if longest is None:
        n = max(len(syms), 2)
        longest = rng.choice([L for L in range(1, cap + 1) if n <= 1 << L])
    while len(syms) < max(2, longest + 1):
        syms.add(rng.choice([s for s in range(size) if s not in syms]))
    syms = sorted(syms)
    out = [0] * size
    for s, l in zip(syms, random_lengths(len(syms), longest, rng)):
        out[s] = l
    return out


def _rle(seq):
    """[(code-length symbol, extra value, lengths covered)]: zero runs as 18 (11 .. 138) and 17 (3 .. 10), others as 16 (3 .. 6)"""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        v, run = seq[i], j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11, k)); run -= k
            if run >= 3:
                out.append((17, run - 3, run)); run = 0
        else:
            out.append((v, 0, 1)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3, k)); run -= k
        out += [(v, 0, 1)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _token_symbols(tokens):
    ll, d = set(), set()
    for t in tokens:
        if isinstance(t, int):
            ll.add(t)
        elif t[0] == "ll":
            ll.add(t[1])
        elif t[0] == "d":
            d.add(t[1])
        elif t[0] != "bits":
            ll.add(len_symbol(t[0], len(t) > 2 and t[2])[0]); d.add(dist_symbol(t[1])[0])
    return ll, d


def _write_tokens(b, blk, ll_code, d_code, out, raw, rec):
    toks = []
    for t in blk["tokens"]:
        p0 = b.nbits
        if isinstance(t, int):
            b.code(*ll_code[t]); out.append(t)
            toks.append((p0, b.nbits))
        elif t[0] == "ll":
            assert raw; b.code(*ll_code[t[1]]); toks.append((p0, b.nbits))
        elif t[0] == "d":
            assert raw; b.code(*d_code[t[1]]); toks.append((p0, b.nbits))
        elif t[0] == "bits":
            assert raw; b.put(t[1], t[2]); toks.append((p0, b.nbits))
        else:
            length, dist = t[0], t[1]
            ls, lv, lb = len_symbol(length, len(t) > 2 and t[2])
            ds, dv, db = dist_symbol(dist)
            b.code(*ll_code[ls]); p1 = b.nbits
            b.put(lv, lb); p2 = b.nbits
            b.code(*d_code[ds]); p3 = b.nbits
            b.put(dv, db)
            assert raw or dist <= len(out), (dist, len(out))
            for _ in range(length):                                     # byte by byte: a source byte may be one this match wrote
                out.append(out[-dist] if dist <= len(out) else 0)
            toks.append((p0, p1, p2, p3, b.nbits))                      # start, after the length code, its extra bits, the distance code, end
    rec["tokens"] = toks
    if blk["eob"]:
        rec["eob"] = (b.nbits, b.nbits + ll_code[256][1])
        b.code(*ll_code[256])
    else:
        assert raw


def _valid_code(lens, strict):
    k, n = kraft(lens), sum(1 for l in lens if l)
    return k == 32768 or (not strict and (n == 0 or (n == 1 and max(lens) == 1)))


def _write_dynamic(b, blk, out, raw, rec):
    rng = random.Random(blk["seed"])
    used_ll, used_d = _token_symbols(blk["tokens"])
    used_ll.add(256)
    if blk["ll_lens"] is not None:
        ll = _as_list(blk["ll_lens"], 288)
    elif len(used_ll) == 1 and not blk["full"] and blk["ll_max"] in (None, 1):
        ll = _as_list({256: 1}, 288)                                    # an empty block: the end-of-block code alone, one bit
    else:
        ll = _generate(used_ll, 286, blk["ll_max"], blk["full"], rng) + [0, 0]
    if blk["d_lens"] is not None:
        d = _as_list(blk["d_lens"], 32)
    elif not used_d and not blk["full"] and blk["d_max"] is None:
        d = [0] * 32                                                    # no distance code at all
    elif len(used_d) == 1 and not blk["full"] and blk["d_max"] in (None, 1):
        d = _as_list({min(used_d): 1}, 32)                              # the single distance code of one bit
    else:
        d = _generate(used_d, 30, blk["d_max"], blk["full"], rng) + [0, 0]
    hlit = blk["hlit"] or max(257, max(s for s in range(288) if ll[s]) + 1 if any(ll) else 257)
    hdist = blk["hdist"] or max(1, max(s for s in range(32) if d[s]) + 1 if any(d) else 1)
    assert raw or (257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(ll[hlit:]) and not any(d[hdist:])), (hlit, hdist)
    assert 257 <= hlit <= 288 and 1 <= hdist <= 32
    if blk.get("cl_syms") is not None:
        cls = list(blk["cl_syms"])                                      # raw: the header's symbols as given
    elif blk["form"] == "plain":
        cls = [(l, 0, 1) for l in ll[:hlit] + d[:hdist]]
    elif blk["form"] == "greedy":
        cls = _rle(ll[:hlit]) + _rle(d[:hdist])
    else:
        assert blk["form"] in ("cross", "maximal"), blk["form"]
        cls = _rle(ll[:hlit] + d[:hdist])
    if blk["form"] == "maximal":
        assert (18, 127, 138) in cls and any(a == c == (16, 3, 6) for a, c in zip(cls, cls[1:]))
    used_cl = {c[0] for c in cls}
    if blk["cl_lens"] is not None:
        cl = _as_list(blk["cl_lens"], 19)
    else:
        cl = _generate(used_cl, 19, blk["cl_max"], False, rng, cap=7)
    order_last = max([i for i in range(19) if cl[CL_ORDER[i]]] + [3]) + 1
    hclen = blk["hclen"] or order_last
    assert 4 <= hclen <= 19 and (raw or hclen >= order_last)
    if not raw:
        assert _valid_code(ll[:hlit], False) and _valid_code(d[:hdist], False) and _valid_code(cl, True) and ll[256]
        assert all(ll[s] for s in used_ll) and all(d[s] for s in used_d) and max(used_ll) < 286 and max(used_d | {0}) < 30
        assert sum(c[2] for c in cls) == hlit + hdist
    b.put(hlit - 257, 5); b.put(hdist - 1, 5); b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl[CL_ORDER[i]], 3)
    cl_code = canonical(cl)
    for s, v, _ in cls:
        b.code(*cl_code[s])
        if s >= 16:
            b.put(v, CL_EXTRA[s])
    rec.update(ll_lens=ll[:hlit], d_lens=d[:hdist], cl_lens=cl, hlit=hlit, hdist=hdist, hclen=hclen, cl_syms=cls, header_end=b.nbits)
    _write_tokens(b, blk, canonical(ll), canonical(d), out, raw, rec)


def build(blocks, raw=False, info=None):
    """(deflate bytes, expected output).  The last block is the final one unless a block says otherwise (final=True / False).
    info: a list that receives one dict per block: kind, start and end (bit positions), and for Huffman blocks the token
    positions; for dynamic blocks the lengths and the header's code-length symbols as well."""
    b, out = Bits(), bytearray()
    for k, blk in enumerate(blocks):
        final = blk["final"] if blk["final"] is not None else k == len(blocks) - 1
        assert raw or final == (k == len(blocks) - 1)
        rec = dict(kind=blk["kind"], start=b.nbits, final=final)
        b.put(int(final), 1)
        if blk["kind"] == "stored":
            b.put(0, 2); b.align()
            n = len(blk["payload"])
            assert n <= 65535
            b.put(n, 16); b.put(blk.get("nlen", n ^ 0xffff), 16)
            b.buf += blk["payload"]; out += blk["payload"]
        elif blk["kind"] == "fixed":
            b.put(1, 2)
            _write_tokens(b, blk, canonical(FIXED_LL), canonical(FIXED_D), out, raw, rec)
        else:
            b.put(2, 2)
            _write_dynamic(b, blk, out, raw, rec)
        rec["end"] = b.nbits
        if info is not None:
            info.append(rec)
    assert raw or len(out) <= 65536
    return b.bytes(), bytes(out)


def check(deflate, data):
    """the second reference: zlib takes the stream to its exact end and gives the builder's bytes"""
    d = zlib.decompressobj(-15)
    got = d.decompress(deflate)
    assert d.eof, "zlib did not reach the final block's end"
    assert d.unused_data == b"", "bytes left over after the final block"
    assert got == data, "the builder's expansion and zlib disagree"
    return True


def member(blocks, info=None):
    """a BGZF member of a good stream, validated: (member bytes, expected output)"""
    import inflate_corpus as ic
    dfl, data = build(blocks, info=info)
    check(dfl, data)
    return ic.wrap(dfl, data), data
