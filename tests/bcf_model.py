"""A plain numpy model of the FORMAT part of a BCF record as the host writer (vcfgl_amd/csrc/host/vcf_sink.h) encodes it -- the
specification of vgl_bcf_encode_device.  Fields, site_status and n_alleles in, bytes and site offsets out.

For every kept site (site_status >= 0) and every field, in the order given:
    the typed key       0x11 id (id <= 127), 0x12 + 2 bytes (<= 32767), 0x13 + 4 bytes
    the size/type       (n << 4 | bt) for n < 15, 0xF0 | bt followed by the typed integer n for n >= 15; n = 0: bt alone, no values
    n * N values        integers in int8 (max <= 127 and min >= -120), int16 (max <= 32767 and min >= -32760) or int32, the range taken
                        over the ordinary values only (a vector without one is int8); missing -> 0x80 / 0x8000 / unchanged, vector end
                        -> 0x81 / 0x8001 / unchanged; float32 as bit patterns; little endian
A field's tensor is [n_sites, stride] (int32 or float32), value k of sample s of site i at [i, s * n(i) + k], n(i) = 1 (ONE),
nA (nA + 1) / 2 (PER_G) or nA (PER_A) with nA = n_alleles[i], never more than stride // N.
"""
import numpy as np

ONE, PER_G, PER_A = 0, 1, 2
INT32_MISSING = -(2 ** 31)
INT32_VEND = INT32_MISSING + 1
FLOAT_MISSING_BITS = 0x7F800001
BT_INT8, BT_INT16, BT_INT32, BT_FLOAT = 1, 2, 3, 5


def enc_int1(v):
    v = int(v)
    if v <= 127:
        return bytes([0x11, v])
    if v <= 32767:
        return bytes([0x12]) + v.to_bytes(2, "little")
    return bytes([0x13]) + v.to_bytes(4, "little")


def enc_size(n, bt):
    if n < 15:
        return bytes([n << 4 | bt])
    return bytes([0xF0 | bt]) + enc_int1(n)


def int_type(values):
    v = np.asarray(values, dtype=np.int64).ravel()
    v = v[(v != INT32_MISSING) & (v != INT32_VEND)]
    if v.size == 0:
        return BT_INT8
    mn, mx = int(v.min()), int(v.max())
    if mx <= 127 and mn >= -120:
        return BT_INT8
    if mx <= 32767 and mn >= -32760:
        return BT_INT16
    return BT_INT32


def enc_ints(values, bt):
    v = np.asarray(values, dtype=np.int32).ravel()
    if bt == BT_INT32:
        return v.astype("<i4").tobytes()
    miss, vend = v == INT32_MISSING, v == INT32_VEND
    if bt == BT_INT8:
        o = v.astype(np.int64).astype(np.uint8)                      # (the low byte)
        o[miss], o[vend] = 0x80, 0x81
        return o.tobytes()
    o = (v.astype(np.int64) & 0xFFFF).astype("<u2")
    o[miss], o[vend] = 0x8000, 0x8001
    return o.tobytes()


def encode_int_field(key_id, n, values):
    """one integer field: what `vcfgl_hip --encode-ints <key id> <n> <values>` prints"""
    bt = int_type(values)
    return enc_int1(key_id) + enc_size(n, bt) + enc_ints(values, bt)


def values_of(kind, nA, stride, N):
    n = nA * (nA + 1) // 2 if kind == PER_G else nA if kind == PER_A else 1
    fit = stride // N if N > 0 else 0
    return max(0, min(n, fit))


def encode(fields, site_status, n_alleles, N):
    """fields = [(key id, array [n_sites, stride] int32 / float32, ONE / PER_G / PER_A)] -> (bytes, int64 offsets [n_sites + 1])"""
    out = bytearray()
    off = [0]
    for i, (st, nA) in enumerate(zip(site_status, n_alleles)):
        if st >= 0:
            for key_id, arr, kind in fields:
                n = values_of(kind, int(nA), arr.shape[1], N)
                vals = arr[i, :n * N]
                out += enc_int1(key_id)
                if arr.dtype == np.float32:
                    out += enc_size(n, BT_FLOAT) + vals.view(np.uint32).astype("<u4").tobytes()
                else:
                    bt = int_type(vals)
                    out += enc_size(n, bt) + enc_ints(vals, bt)
        off.append(len(out))
    return bytes(out), np.array(off, dtype=np.int64)


# the values at which the integer type changes, on both sides, and the special vectors of the specification
THRESHOLDS = [127, 128, -120, -121, 32767, 32768, -32760, -32761, INT32_MISSING + 2, 2 ** 31 - 1]


def threshold_vectors():
    """[(name, [values])]: each threshold value beside small ordinary values, and the vectors without an ordinary value"""
    out = [("t%d" % t, [0, t, 5]) for t in THRESHOLDS]
    out += [("all missing", [INT32_MISSING] * 3), ("only vector end", [INT32_VEND] * 3),
            ("mixed", [7, INT32_MISSING, INT32_VEND, -3, 100]), ("mixed16", [300, INT32_MISSING, INT32_VEND, -3]),
            ("mixed32", [70000, INT32_MISSING, INT32_VEND, -3])]
    return out
