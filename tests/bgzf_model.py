"""A bit-exact reference model of one BGZF member of the device compressor (vgl_bgzf.hip, k_bgzf_member), and a strict inflater.

The model is the specification of the device's output: plain Python / numpy written from the kernel's documented rules, no floating
point, no order.  member(data) returns the member's bytes (gzip header with the BC field, deflate data, CRC32, ISIZE) and every
intermediate result: the tokens, histograms, code lengths (and the Huffman depth before the 15 / 7-bit limit), the three block
sizes, the chosen mode and each parse segment's bit count.

  * LZ77 candidates: hash3 = ((b0 | b1 << 8 | b2 << 16) * 2654435761 mod 2^32) >> 20, defined where p + 2 < len.  The wavefront
    candidate of p is the nearest earlier position of the same aligned group of 64 positions with the same hash; the table
    candidate is the latest position with that hash before the group starts, usable at distance <= 32768.  Their common
    prefixes with p, on the first min(32, len - p) bytes, decide: the wavefront candidate when its length is >= 3 and not below
    the table's, else the table's when its length is >= 3, else none.
  * Parse: segments of 512 positions, greedy, a match ends at its segment's end and at 258 bytes; one-byte lazy rule (zlib): a
    match shorter than 32 becomes a literal when the next position (inside the segment) has a strictly longer one.
  * Codes: end-of-block counted once; Moffat-Katajainen code lengths of the weights sorted by (weight, symbol), then the
    length limit (clamp, then: one code fewer at the limit, the deepest shorter code split, until the Kraft sum is 1), the
    longest codes to the rarest symbols; fewer than two used symbols are completed with the first unused ones (weight 1).
  * Header: HLIT / HDIST trimmed to the last nonzero length (at least 257 / 1), one run-length sequence over both alphabets
    (runs cross from one into the other), 18 / 17 for zero runs, 16 after one explicit copy of a nonzero length; HCLEN trimmed
    in RFC 1951 order (at least 4).
  * Mode: dynamic unless fixed is strictly smaller in bits; stored (5 + len bytes) when strictly smaller than the chosen one
    in whole bytes.  Padding bits are zero.

inflate(raw) decodes raw deflate data independently (RFC 1951 only, nothing shared with the model) and asserts one final block,
complete codes (Kraft sum exactly 1), lengths <= 15 (<= 7 for the code-length code), no symbol 286/287 or distance 30/31,
distances within 32768 and the output so far, consistent LEN/NLEN, zero padding and no trailing bytes."""
import heapq
import struct
import zlib

import numpy as np

MEMBER = 0xff00
SEG = 512
HASH_BITS = 12
MAX_DIST = 32768
GZ_HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EB = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EB = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _symbol_tables():
    lsym = np.zeros(259, np.int64)
    for i, b in enumerate(LEN_BASE):
        lsym[b:b + (1 << LEN_EB[i])] = 257 + i
    lsym[258] = 285                                      # (284 with extra 31 would also say 258; deflate uses 285)
    dsym = np.zeros(MAX_DIST + 1, np.int64)
    for i, b in enumerate(DIST_BASE):
        dsym[b:b + (1 << DIST_EB[i])] = i
    return lsym, dsym


LSYM, DSYM = _symbol_tables()
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def len_extra(l):
    s = int(LSYM[l])
    return s, LEN_EB[s - 257], l - LEN_BASE[s - 257]


def dist_extra(d):
    s = int(DSYM[d])
    return s, DIST_EB[s], d - DIST_BASE[s]


# ---- LZ77 ----------------------------------------------------------------------------------------------------------------------
def hash3(b):
    """hash of the 3 bytes at every p with p + 2 < len (uint8 array in)"""
    b = b.astype(np.uint64)
    v = b[:-2] | b[1:-1] << np.uint64(8) | b[2:] << np.uint64(16)
    return ((v * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HASH_BITS)


def _lcp(pad, c, p, cap, step=32):
    """common prefix of [c, ...) and [p, ...), at most cap (arrays), in chunks of `step` bytes"""
    out = np.zeros(len(p), np.int64)
    live = np.arange(len(p))
    k0 = 0
    kmax = int(cap.max()) if len(cap) else 0
    while len(live) and k0 < kmax:
        k = np.arange(k0, k0 + step)
        eq = pad[c[live, None] + k] == pad[p[live, None] + k]
        full = eq.all(1)
        first = np.where(full, step, eq.argmin(1))
        out[live] = k0 + first
        live = live[full & (k0 + step < cap[live])]
        k0 += step
    return np.minimum(out, cap)


def candidates(b):
    """per position: the distance the candidate stage keeps (0: none), and the full match length there (<= 258, <= len - p)"""
    n = len(b)
    dist = np.zeros(n, np.int64)
    full = np.zeros(n, np.int64)
    nh = max(n - 2, 0)
    if nh == 0:
        return dist, full
    pad = np.concatenate([b, np.zeros(320, np.uint8)])
    h = hash3(b).astype(np.int64)
    pos = np.arange(nh, dtype=np.int64)
    grp = pos >> 6
    # wavefront candidate: the previous position of the same (group, hash)
    order = np.lexsort((pos, h, grp))
    same = (grp[order][1:] == grp[order][:-1]) & (h[order][1:] == h[order][:-1])
    wc = np.full(nh, -1, np.int64)
    wc[order[1:][same]] = order[:-1][same]
    # table candidate: the latest position with the same hash before the group starts
    keys = np.sort(h << 17 | pos)
    i = np.searchsorted(keys, h << 17 | grp << 6, side="left") - 1
    ok = i >= 0
    ok[ok] = (keys[i[ok]] >> 17) == h[ok]
    tc = np.where(ok, keys[np.maximum(i, 0)] & ((1 << 17) - 1), -1)
    tc = np.where(pos - tc <= MAX_DIST, tc, -1)
    lim = np.minimum(n - pos, 32)
    lw = np.zeros(nh, np.int64)
    m = wc >= 0
    lw[m] = _lcp(pad, wc[m], pos[m], lim[m])
    lt = np.zeros(nh, np.int64)
    m = tc >= 0
    lt[m] = _lcp(pad, tc[m], pos[m], lim[m])
    use_w = (lw >= 3) & (lw >= lt)
    use_t = ~use_w & (lt >= 3)
    dist[:nh] = np.where(use_w, pos - wc, np.where(use_t, pos - tc, 0))
    m = np.nonzero(dist)[0]
    full[m] = _lcp(pad, m - dist[m], m, np.minimum(258, n - m))
    return dist, full


def parse(b, dist, full):
    """tokens (p, length, distance), length 0 for a literal"""
    n = len(b)
    dl, fl = dist.tolist(), full.tolist()
    toks = []
    for s0 in range(0, n, SEG):
        s1 = min(s0 + SEG, n)
        p = s0
        while p < s1:
            l = min(fl[p], s1 - p)
            if 3 <= l < 32 and p + 1 < s1 and min(fl[p + 1], s1 - p - 1) > l:
                l = 0                                     # lazy: a longer match one byte on
            if l >= 3:
                toks.append((p, l, dl[p]))
                p += l
            else:
                toks.append((p, 0, 0))
                p += 1
    return toks


# ---- Huffman codes -----------------------------------------------------------------------------------------------------------
def build_lengths(freq, maxbits):
    """(lengths, unconstrained depth, repair steps): minimum-redundancy lengths limited to maxbits, as the device builds them"""
    n = len(freq)
    w = [int(f) for f in freq]
    used = sum(1 for f in w if f)
    for s in range(n):
        if used >= 2:
            break
        if not w[s]:
            w[s] = 1
            used += 1
    syms = sorted((s for s in range(n) if w[s]), key=lambda s: (w[s], s))
    A = [w[s] for s in syms]
    m = len(A)
    # Moffat & Katajainen (1995), in place on the ascending weights
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or A[root] < A[leaf]:
            A[nxt] = A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] = A[leaf]; leaf += 1
        if leaf >= m or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] += A[leaf]; leaf += 1
    A[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, usedn, dpth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            usedn += 1; root -= 1
        while avbl > usedn:
            A[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl, dpth, usedn = 2 * usedn, dpth + 1, 0
    depth = max(A)
    # length limit: clamp, then bring the Kraft sum back to exactly 1
    cnt = [0] * (maxbits + 1)
    for a in A:
        cnt[min(a, maxbits)] += 1
    total = sum(cnt[i] << (maxbits - i) for i in range(1, maxbits + 1))
    steps = 0
    while total != 1 << maxbits:
        cnt[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if cnt[i]:
                cnt[i] -= 1; cnt[i + 1] += 2
                break
        total -= 1
        steps += 1
    lens = [0] * n
    j = 0
    for i in range(maxbits, 0, -1):
        for _ in range(cnt[i]):
            lens[syms[j]] = i
            j += 1
    return lens, depth, steps


def huffman_cost(weights):
    """cost of an optimal (unlimited) prefix code of the nonzero weights: the sum of all merged weights"""
    h = [int(x) for x in weights if x]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        cost += a
        heapq.heappush(h, a)
    return cost


def canonical(lens):
    """RFC 1951 3.2.2 codes (MSB-first integers)"""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + bl[b - 1]) << 1
        nxt[b] = c
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _rev(c, l):
    return int(format(c, "0%db" % l)[::-1], 2) if l else 0


def rle(seq):
    """RFC 1951 3.2.7 run-length sequence of code lengths: list of (symbol, extra)"""
    out, i, tot = [], 0, len(seq)
    while i < tot:
        v = seq[i]
        run = 1
        while i + run < tot and seq[i + run] == v:
            run += 1
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11)); run -= r; i += r
            if run >= 3:
                out.append((17, run - 3)); i += run; run = 0
            out += [(0, 0)] * run; i += run
        else:
            out.append((v, 0)); i += 1; run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3)); run -= r; i += r
            out += [(v, 0)] * run; i += run
    return out


RLE_EB = {16: 2, 17: 3, 18: 7}


# ---- bits --------------------------------------------------------------------------------------------------------------------
def _pack(vals, nbits):
    """LSB-first concatenation of (value, nbits) pairs, zero padded to a byte"""
    vals = np.asarray(vals, np.int64)
    nbits = np.asarray(nbits, np.int64)
    k = np.arange(16)
    bits = ((vals[:, None] >> k) & 1).astype(np.uint8)
    return np.packbits(bits[k[None, :] < nbits[:, None]], bitorder="little").tobytes()


class Member:
    """one member: .raw (bytes), .deflate, .tokens, .hist_ll / .hist_d / .cl_hist, .len_ll / .len_d / .len_cl, .depth and
    .repair (per alphabet 'll', 'd', 'cl'), .hlit / .hdist / .hclen, .rle, .bits ({0: stored, 1: fixed, 2: dynamic}), .mode,
    .seg_bits (per segment, the end-of-block code not included)"""


def member(data, force_mode=None):
    b = np.frombuffer(bytes(data), np.uint8)
    n = len(b)
    assert 1 <= n <= MEMBER
    M = Member()
    dist, full = candidates(b)
    toks = parse(b, dist, full)
    M.tokens = toks
    hist_ll, hist_d = [0] * 286, [0] * 30
    for p, l, d in toks:
        if l:
            hist_ll[LSYM[l]] += 1
            hist_d[DSYM[d]] += 1
        else:
            hist_ll[b[p]] += 1
    hist_ll[256] = 1
    M.hist_ll, M.hist_d = hist_ll, hist_d
    len_ll, dll, rll = build_lengths(hist_ll, 15)
    len_d, dd, rd = build_lengths(hist_d, 15)
    hlit = 286
    while hlit > 257 and not len_ll[hlit - 1]:
        hlit -= 1
    hdist = 30
    while hdist > 1 and not len_d[hdist - 1]:
        hdist -= 1
    seq = rle(len_ll[:hlit] + len_d[:hdist])
    cl_hist = [0] * 19
    for s, _ in seq:
        cl_hist[s] += 1
    len_cl, dcl, rcl = build_lengths(cl_hist, 7)
    hclen = 19
    while hclen > 4 and not len_cl[CL_ORDER[hclen - 1]]:
        hclen -= 1
    M.len_ll, M.len_d, M.len_cl, M.cl_hist, M.rle = len_ll, len_d, len_cl, cl_hist, seq
    M.hlit, M.hdist, M.hclen = hlit, hdist, hclen
    M.depth = {"ll": dll, "d": dd, "cl": dcl}
    M.repair = {"ll": rll, "d": rd, "cl": rcl}

    extra = sum(f * (LEN_EB[s - 257] if s >= 257 else 0) for s, f in enumerate(hist_ll)) + sum(f * DIST_EB[s] for s, f in enumerate(hist_d))
    hdr = 3 + 5 + 5 + 4 + 3 * hclen + sum(len_cl[s] + RLE_EB.get(s, 0) for s, _ in seq)
    dyn = hdr + sum(f * l for f, l in zip(hist_ll, len_ll)) + sum(f * l for f, l in zip(hist_d, len_d)) + extra
    fix = 3 + sum(f * FIXED_LL[s] for s, f in enumerate(hist_ll)) + 5 * sum(hist_d) + extra
    stored = 8 * (5 + n)
    M.bits = {0: stored, 1: fix, 2: dyn}
    mode, best = 2, dyn
    if fix < best:
        mode, best = 1, fix
    if stored < (best + 7) // 8 * 8:
        mode = 0
    if force_mode is not None:
        mode = force_mode
    M.mode = mode

    if mode == 0:
        deflate = bytes([1]) + struct.pack("<HH", n, n ^ 0xffff) + bytes(b)
        M.seg_bits = None
    else:
        ll, dl_ = (FIXED_LL, FIXED_D) if mode == 1 else (len_ll, len_d)
        cll, cd = canonical(ll), canonical(dl_)
        rll_ = [_rev(c, l) for c, l in zip(cll, ll)]
        rd_ = [_rev(c, l) for c, l in zip(cd, dl_)]
        vals, nb = [], []

        def put(v, k):
            vals.append(v); nb.append(k)
        if mode == 1:
            put(1 | 1 << 1, 3)
        else:
            put(1 | 2 << 1, 3); put(hlit - 257, 5); put(hdist - 1, 5); put(hclen - 4, 4)
            for i in range(hclen):
                put(len_cl[CL_ORDER[i]], 3)
            ccl = canonical(len_cl)
            for s, x in seq:
                put(_rev(ccl[s], len_cl[s]), len_cl[s])
                if s >= 16:
                    put(x, RLE_EB[s])
        hdr_bits = sum(nb)
        seg_bits = [0] * ((n + SEG - 1) // SEG)
        for p, l, d in toks:
            k0 = len(nb)
            if l:
                s, ne, ex = len_extra(l)
                put(rll_[s], ll[s]); put(ex, ne)
                s, ne, ex = dist_extra(d)
                put(rd_[s], dl_[s]); put(ex, ne)
            else:
                put(rll_[b[p]], ll[b[p]])
            seg_bits[p // SEG] += sum(nb[k0:])
        put(rll_[256], ll[256])
        assert sum(nb) == M.bits[mode]
        M.hdr_bits, M.seg_bits = hdr_bits, seg_bits
        deflate = _pack(vals, nb)
    M.deflate = deflate
    size = 18 + len(deflate) + 8
    # (a forced mode can exceed BSIZE's 65536: then no member bytes)
    M.raw = GZ_HEADER + struct.pack("<H", size - 1) + deflate + struct.pack("<II", zlib.crc32(bytes(b)), n) if size <= 65536 else None
    return M


def compress(data):
    """the model's BGZF stream of data (no EOF member): members of 0xff00 input bytes"""
    data = bytes(data)
    return b"".join(member(data[i:i + MEMBER]).raw for i in range(0, len(data), MEMBER))


def split_members(raw):
    """the members of a BGZF stream, by their BSIZE fields"""
    out, off = [], 0
    while off < len(raw):
        assert raw[off:off + 4] == b"\x1f\x8b\x08\x04" and raw[off + 12:off + 14] == b"BC", off
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        out.append(raw[off:off + bsize])
        off += bsize
    assert off == len(raw)
    return out


# ---- strict inflater (RFC 1951, written apart from the model) ----------------------------------------------------------------
class _Bits:
    def __init__(self, raw):
        bits = np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little")
        self.nbits = len(bits)
        padded = np.concatenate([bits, np.zeros(16, np.uint8)]).astype(np.int64)
        self.win = (np.lib.stride_tricks.sliding_window_view(padded, 16)[:self.nbits + 1] << np.arange(16)).sum(1).tolist()
        self.pos = 0

    def get(self, k):
        assert self.pos + k <= self.nbits, "read past the end of the data"
        v = self.win[self.pos] & ((1 << k) - 1) if k else 0
        self.pos += k
        return v


def _decoder(lens, maxbits, what):
    """a 2^15-entry table of (symbol, length) over the next 15 bits; asserts a complete code within maxbits"""
    assert all(0 <= l <= maxbits for l in lens), (what, "length over", maxbits)
    kraft = sum(1 << (15 - l) for l in lens if l)
    assert kraft == 1 << 15, (what, "incomplete or oversubscribed code", kraft / (1 << 15))
    bl = [0] * 16
    for l in lens:
        if l:
            bl[l] += 1
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + bl[l - 1]) << 1
        nxt[l] = code
    tab = [None] * (1 << 15)
    for s, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]; nxt[l] += 1
        r = int(format(c, "0%db" % l)[::-1], 2)
        for j in range(r, 1 << 15, 1 << l):
            tab[j] = (s, l)
    return tab


def _sym(bs, tab):
    s, l = tab[bs.win[bs.pos] & 0x7fff]
    bs.get(l)
    return s


def inflate(raw):
    """decode one final deflate block strictly: dict(btype, len_ll, len_d, len_cl, hlit, hdist, hclen, tokens, out)"""
    bs = _Bits(bytes(raw))
    final, btype = bs.get(1), bs.get(2)
    assert final == 1, "not a single final block"
    assert btype != 3, "BTYPE 11"
    r = {"btype": btype, "tokens": []}
    out = bytearray()
    if btype == 0:
        bs.get((-bs.pos) % 8)
        ln, nln = bs.get(16), bs.get(16)
        assert ln ^ nln == 0xffff, "LEN / NLEN"
        assert bs.pos + 8 * ln == bs.nbits, "stored length against the data"
        i = bs.pos // 8
        out += raw[i:i + ln]
        bs.pos += 8 * ln
        r["out"] = bytes(out)
        return r
    if btype == 1:
        len_ll, len_d = FIXED_LL, FIXED_D
    else:
        hlit, hdist, hclen = bs.get(5) + 257, bs.get(5) + 1, bs.get(4) + 4
        assert hlit <= 286 and hdist <= 30, ("HLIT / HDIST", hlit, hdist)
        len_cl = [0] * 19
        for i in range(hclen):
            len_cl[CL_ORDER[i]] = bs.get(3)
        tcl = _decoder(len_cl, 7, "code-length code")
        seq = []
        while len(seq) < hlit + hdist:
            s = _sym(bs, tcl)
            if s < 16:
                seq.append(s)
            elif s == 16:
                assert seq, "repeat with no previous length"
                seq += [seq[-1]] * (3 + bs.get(2))
            elif s == 17:
                seq += [0] * (3 + bs.get(3))
            else:
                seq += [0] * (11 + bs.get(7))
        assert len(seq) == hlit + hdist, "a run crosses the end of the lengths"
        len_ll, len_d = seq[:hlit], seq[hlit:]
        assert len_ll[256], "no end-of-block code"
        r.update(hlit=hlit, hdist=hdist, hclen=hclen, len_cl=len_cl)
    r["len_ll"], r["len_d"] = list(len_ll), list(len_d)
    tll = _decoder(len_ll, 15, "literal/length code")
    td = _decoder(len_d, 15, "distance code")
    toks = r["tokens"]
    while True:
        s = _sym(bs, tll)
        if s < 256:
            out.append(s)
            toks.append((s,))
            continue
        if s == 256:
            break
        assert s < 286, ("literal/length symbol", s)
        l = LEN_BASE[s - 257] + bs.get(LEN_EB[s - 257])
        ds = _sym(bs, td)
        assert ds < 30, ("distance symbol", ds)
        d = DIST_BASE[ds] + bs.get(DIST_EB[ds])
        assert d <= MAX_DIST and d <= len(out), ("distance", d, len(out))
        for _ in range(l):
            out.append(out[-d])
        toks.append((l, d))
    assert bs.nbits - bs.pos < 8, "bytes after the final block"
    assert bs.get(bs.nbits - bs.pos) == 0, "nonzero padding"
    r["out"] = bytes(out)
    return r


def inflate_member(raw):
    """strictly decode one BGZF member (header, BSIZE, CRC32, ISIZE) and return inflate()'s dict"""
    raw = bytes(raw)
    assert raw[:16] == GZ_HEADER, raw[:16]
    assert struct.unpack_from("<H", raw, 16)[0] + 1 == len(raw) <= 65536
    r = inflate(raw[18:-8])
    crc, isize = struct.unpack_from("<II", raw, len(raw) - 8)
    assert crc == zlib.crc32(r["out"]) and isize == len(r["out"]), "CRC32 / ISIZE"
    return r


# ---- corpus builders -----------------------------------------------------------------------------------------------------------
def _tri(o, q):
    return o[q] | o[q + 1] << 8 | o[q + 2] << 16


def _h(v):
    return (v * 2654435761 & 0xffffffff) >> (32 - HASH_BITS)


def chain(k, margin):
    """k weights where each is the sum of all lighter ones plus `margin`: a Huffman tree of depth k - 1 even with a few stray
    counts of total weight <= margin added"""
    w = [1, 1]
    while len(w) < k:
        w.append(sum(w[:-1]) + margin)
    return w


def laid_out(seed, dcodes, margin, lcodes=None, n=MEMBER):
    """one member of matches laid out by hand: distance codes `dcodes` with chain() counts (rarest nearest), and with `lcodes`
    length codes with chain() counts (rarest longest).  Every copy's source is the latest position with its hash, and neither
    the bytes around a copy nor the byte that ends it form a 3-byte string seen before, so the parse takes exactly these
    matches and no others."""
    rng = np.random.default_rng(seed)
    dseq = np.repeat(list(dcodes), chain(len(dcodes), margin))
    rng.shuffle(dseq)
    if lcodes is not None:
        lseq = np.repeat(list(lcodes), chain(len(lcodes), margin)[::-1])
        rng.shuffle(lseq)
    top = dcodes[-1]
    out = bytearray(rng.integers(0, 256, DIST_BASE[top] + (1 << DIST_EB[top]), dtype=np.uint8).tobytes())
    last, seen, done = {}, set(), 0

    def fin():
        nonlocal done
        while done + 2 < len(out):
            v = _tri(out, done)
            last[_h(v)] = done
            seen.add(v)
            done += 1
    fin()
    for i, c in enumerate(dseq.tolist()):
        L = 3
        if lcodes is not None:
            k = int(lseq[i % len(lseq)]) - 257
            L = LEN_BASE[k] + int(rng.integers(0, 1 << LEN_EB[k]))
        p = len(out)
        for d in (DIST_BASE[c] + rng.permutation(1 << DIST_EB[c])[:32]).tolist():
            s = p - d
            if d <= L or last.get(_h(_tri(out, s))) != s:
                continue
            if (out[p - 2] | out[p - 1] << 8 | out[s] << 16) not in seen and (out[p - 1] | out[s] << 8 | out[s + 1] << 16) not in seen:
                break
        else:
            continue
        for _ in range(L):
            out.append(out[-d])
        for e in rng.permutation(256).tolist():
            if e != out[s + L] and (out[-2] | out[-1] << 8 | e << 16) not in seen:
                break
        out.append(e)
        fin()
        if len(out) >= n:
            break
    return bytes(out[:n])


def code_ends():
    """(length, distance) pairs: every length code and every distance code at both ends of its extra-bits range"""
    lens = sorted({x for i, b in enumerate(LEN_BASE) for x in (b, min(b + (1 << LEN_EB[i]) - 1, 257 if i < 28 else 258))})
    dists = sorted({x for i, b in enumerate(DIST_BASE) for x in (b, b + (1 << DIST_EB[i]) - 1)})
    return [(l, 600) for l in lens] + [(3, d) for d in dists]


def islands(seed, pairs):
    """matches of exactly (length, distance) each: a random island, zeros, and its copy at the start of a parse segment"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    for L, D in pairs:
        if D <= L:                                        # distances 1, 2 (and 3 with length 3): a short period
            while True:
                unit = rng.integers(1, 256, D, dtype=np.uint8).tobytes()
                if len(set(unit)) == D:
                    break
            body = unit * ((L + D) // D + 1)
            body = body[:D + L] + bytes([unit[(L) % D] ^ 0x80])
            start = -(-(len(out) + 1) // SEG) * SEG - D
            if start // MEMBER != (start + len(body)) // MEMBER or start < len(out):
                start += SEG
            out += bytes(start - len(out)) + body
            continue
        while True:
            isl = rng.integers(1, 256, L + 2, dtype=np.uint8).tobytes()
            hs = [_h(_tri(isl, q)) for q in range(L)] + [_h(isl[-2] | isl[-1] << 8), _h(isl[-1]), 0]
            if hs.count(hs[0]) == 1:
                break
        p = -(-(len(out) + 1 + D) // SEG) * SEG
        if (p - D - 1) // MEMBER != (p + L + 1) // MEMBER:
            p = -(-(len(out) + 1) // MEMBER) * MEMBER + -(-(D + 1) // SEG) * SEG
        out += bytes(p - D - 1 - len(out)) + isl
        out += bytes(p - len(out)) + isl[1:L + 1] + bytes([isl[L + 1] ^ 0x55])
    return bytes(out)


def corpus():
    """name -> bytes: the shapes of the device tests, text, runs, periods, random bytes and the built inputs"""
    rng = np.random.default_rng(20261016)
    c = {}
    t = rng.integers(0, 40, 4000)
    c["vcf_text"] = b"".join(b"chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT:DP\t0/1:%d\n" % (i, x) for i, x in enumerate(t))[:MEMBER + 4321]
    words = [b"0/0", b"0/1", b"1/1", b"-0.30103", b"-1.2", b"\t", b"\n", b"PASS"]
    c["words"] = b"".join(words[i] for i in rng.integers(0, len(words), 40000))[:2 * MEMBER - 77]
    c["random"] = rng.integers(0, 256, MEMBER + 999, dtype=np.uint8).tobytes()
    c["zeros"] = bytes(MEMBER + 5)
    a = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, 32769, dtype=np.uint8).tobytes()
    c["dist_32768_32769"] = (a + a[:20000]) + (b + b[:12000])
    c["periods_runs"] = b"".join(bytes([i % 7]) * (i * 37 % 600 + 1) + bytes(range(i % 256)) for i in range(120))
    c["bcf_like"] = b"".join(struct.pack("<iiHHf", i, rng.integers(0, 60), rng.integers(0, 3), 0x0201, rng.random()) for i in range(5000))
    c["code_ends"] = islands(1, code_ends())
    c["deep_dist"] = laid_out(0, range(3, 20), 8)
    c["deep_cl"] = laid_out(2, range(3, 18), 2, range(257, 276))
    return c
