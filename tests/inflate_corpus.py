"""BGZF members for the inflater's tests: what Python's zlib writes under every setting that changes the shape of a deflate stream,
what the compressor's model (bgzf_model.member) writes in its three forms, the container's edge cases -- and damaged variants of
good members, each still a whole BGZF member by its header and BSIZE, which an inflater must refuse.

    good()      [(name, member bytes, the bytes it inflates to)]
    damaged()   [(name, member bytes)]
    stream(ms)  the members' bytes back to back

zlib settings and what they gave when the corpus was put together (one 0xff00-byte buffer of random ACGT): level 6 one final dynamic
block; Z_FIXED BTYPE 01; level 0 two stored blocks, the first non-final; Z_HUFFMAN_ONLY several dynamic blocks and no distance code;
Z_FULL_FLUSH after 1000 bytes an empty stored block between two dynamic blocks; Z_RLE on zeros distance-1 matches only (one
distance code of one bit, overlapping copies)."""
import functools
import struct
import zlib

import numpy as np

import bgzf_model as bm

M = bm.MEMBER
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def wrap(deflate, data, extra=b"", crc=None, isize=None):
    """a BGZF member around raw deflate data; `extra`: subfields in front of 'BC'"""
    xlen = 6 + len(extra)
    size = 12 + xlen + len(deflate) + 8
    assert size <= 65536, size
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\x00" + struct.pack("<H", size - 1) + deflate +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def deflate_of(member):
    """the raw deflate data of a member (any extra field)"""
    xlen = struct.unpack_from("<H", member, 10)[0]
    return member[12 + xlen:-8]


def vcf_text(n_bytes, samples=200, seed=5):
    rng = np.random.default_rng(seed)
    tok = np.array(["0|0", "0|1", "1|0", "1|1"])
    lines, size, pos = [], 0, 0
    while size < n_bytes:
        pos += 1
        ln = "chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t%s\n" % (pos, "\t".join(tok[rng.choice(4, samples, p=[0.85, 0.06, 0.06, 0.03])]))
        lines.append(ln); size += len(ln)
    return "".join(lines).encode()[:n_bytes]


def far_data():
    """the data of test_gpu_bgzf.py::test_matches_at_distance_32768_and_32769: repeats at exactly 32768 and at 32769"""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, 32769, dtype=np.uint8).tobytes()
    data = (a + a[:20000]) + (b + b[:12000])
    return data + data[:3 * M]


@functools.lru_cache(maxsize=None)
def good():
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, M)].tobytes()
    text = vcf_text(65536)
    out = []

    def add(name, dfl, data, **kw):
        assert zlib.decompress(dfl, -15) == data, name
        out.append((name, wrap(dfl, data, **kw), data))
    add("acgt_level6", deflate(acgt), acgt)
    add("acgt_fixed", deflate(acgt, strategy=zlib.Z_FIXED), acgt)
    add("acgt_level0", deflate(acgt, level=0), acgt)
    add("acgt_huffman_only", deflate(acgt, strategy=zlib.Z_HUFFMAN_ONLY), acgt)
    add("acgt_full_flush", deflate(acgt, flush_at=1000), acgt)
    add("zeros_rle", deflate(bytes(M), strategy=zlib.Z_RLE), bytes(M))
    add("vcf_text_level6", deflate(text[:M]), text[:M])
    add("empty", deflate(b""), b"")
    add("one_byte", deflate(b"A"), b"A")
    add("isize_65536", deflate(text), text)
    add("level1_text", deflate(text[:30011], level=1), text[:30011])
    add("level9_text", deflate(text[:M], level=9), text[:M])
    add("subfield_before_bc", deflate(text[:4097]), text[:4097], extra=b"XY\x03\x00abc")
    far = far_data()
    for k in (0, 1):                                                        # distances up to 32768: zlib stops at 32506, the model does not
        piece = far[k * M:(k + 1) * M]
        m = bm.member(piece)
        if k == 0:
            assert max(d for _, l, d in m.tokens if l) == 32768
        out.append(("model_far_%d" % k, m.raw, piece))
        add("zlib_far_%d" % k, deflate(piece), piece)
    small = text[1000:6017]
    for mode in (0, 1, 2):
        m = bm.member(small, force_mode=mode)
        assert m.mode == mode and m.raw is not None
        out.append(("model_mode%d" % mode, m.raw, small))
    out.append(("eof", EOF, b""))
    for name, raw, data in out:
        assert len(raw) <= 65536 and len(data) <= 65536 and struct.unpack_from("<H", raw, raw.index(b"BC\x02\x00") + 4)[0] + 1 == len(raw), name
    first = {name: deflate_of(raw)[0] & 7 for name, raw, _ in out}
    assert first["acgt_level6"] == 5 and first["acgt_fixed"] == 3 and first["acgt_level0"] == 0 and first["acgt_huffman_only"] == 4
    assert (first["model_mode0"], first["model_mode1"], first["model_mode2"]) == (1, 3, 5)
    return tuple(out)


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, k):                       # LSB first (header fields, extra bits)
        self.v |= v << self.n; self.n += k

    def code(self, c, k):                      # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % k)[::-1], 2), k)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _distance_before_start():
    """BFINAL, fixed codes: literal 'A', then length 3 at distance 2 with one byte produced"""
    b = _Bits()
    b.put(1, 1); b.put(1, 2)
    b.code(0x30 + ord("A"), 8)
    b.code(257 - 256, 7); b.code(1, 5)         # length 3 (symbol 257), distance 2 (symbol 1)
    b.code(0, 7)
    return wrap(b.bytes(), b"AAAA")


@functools.lru_cache(maxsize=None)
def damaged():
    g = {name: (raw, data) for name, raw, data in good()}
    out = []

    def redo(raw, dfl=None, crc=None, isize=None):
        """the member again with another deflate part / CRC / ISIZE and a BSIZE that fits"""
        c0, i0 = struct.unpack_from("<II", raw, len(raw) - 8)
        dfl = deflate_of(raw) if dfl is None else dfl
        size = 18 + len(dfl) + 8
        return raw[:16] + struct.pack("<H", size - 1) + dfl + struct.pack("<II", c0 if crc is None else crc, i0 if isize is None else isize)
    dyn, dyn_data = g["acgt_level6"]
    fix, fix_data = g["acgt_fixed"]
    sto, sto_data = g["acgt_level0"]
    d = bytearray(deflate_of(dyn)); d[len(d) // 2] ^= 0x10
    out.append(("bit_flip_in_the_huffman_data", redo(dyn, dfl=bytes(d))))
    out.append(("crc_flipped", redo(dyn, crc=zlib.crc32(dyn_data) ^ 0x00010000)))
    out.append(("isize_plus_1", redo(fix, isize=len(fix_data) + 1)))
    out.append(("isize_minus_1", redo(fix, isize=len(fix_data) - 1)))
    d = bytearray(deflate_of(dyn)); d[0] |= 6
    out.append(("btype_11", redo(dyn, dfl=bytes(d))))
    d = bytearray(deflate_of(sto)); assert d[0] & 7 == 0; d[3] ^= 0x01
    out.append(("len_nlen_mismatch", redo(sto, dfl=bytes(d))))
    out.append(("data_cut_short", redo(dyn, dfl=deflate_of(dyn)[:-10])))
    out.append(("stored_cut_short", redo(sto, dfl=deflate_of(sto)[:-10])))
    out.append(("distance_before_the_start", _distance_before_start()))
    small = fix_data[:100]
    out.append(("more_than_isize", wrap(deflate(small), small[:50])))
    out.append(("more_than_isize_stored", wrap(deflate(small, level=0), small[:50])))
    out.append(("bytes_after_the_final_block", wrap(deflate(small) + b"\0", small)))
    for name, raw in out:
        assert raw[:4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", raw, 16)[0] + 1 == len(raw) <= 65536, name
        isize = struct.unpack_from("<I", raw, len(raw) - 4)[0]
        assert isize <= 65536, name
        try:                                                               # zlib refuses every one of them as a gzip member too
            ok = len(zlib.decompress(raw, 31)) == isize
        except zlib.error:
            ok = False
        assert not ok, name
    return tuple(out)


def stream(members):
    return b"".join(members)


def bgzf_level6(data, n=M):
    """a file's worth of BGZF at zlib level 6: members of n input bytes and the EOF member"""
    data = bytes(data)
    return b"".join(wrap(deflate(data[i:i + n]), data[i:i + n]) for i in range(0, len(data), n)) + EOF
