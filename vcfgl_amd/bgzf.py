"""BGZF compression and inflation on the device (libvcfgl_hip.so, ABI 7: vgl_bgzf_compress_device, vgl_inflate_members_device).

What a rank of a sharded job uses for per-rank compressed output: each rank compresses its own bytes on its own GPU, and since
BGZF members are independent gzip members, the ranks' pieces concatenated in rank order (plus one EOF member) are a valid file.
Every piece but the last must hold a whole number of 0xff00-byte members' worth of input for the file to be the one a single
call would give; any split decompresses to the same bytes.

    pieces = [bgzf.compress(t) for t in chunks]     # device uint8 tensors in, device uint8 tensors out
    bgzf.write_file(path, pieces)                    # pieces + EOF

The other direction: `index(raw)` lists the members of a BGZF stream on the host, `decompress(t)` inflates a stream that lies on a
device, one member per workgroup, and says per member whether the device took it to its exact end (status 0) or leaves it to the
caller's own inflater (status 1: its bytes in the result are unspecified).

    out, status = bgzf.decompress(t)                 # device uint8 tensor in; device uint8 and int32 tensors out
"""
import ctypes as C

import numpy as np

from . import _abi

MEMBER_BYTES = 0xff00
# the empty member that ends every BGZF file (SAMv1 section 4.1.2)
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bound(n: int) -> int:
    """largest compressed size of n input bytes (the stored form of every member)"""
    return int(_abi.load_library().vgl_bgzf_bound(int(n)))


def compress(t):
    """BGZF members of the bytes of `t` (a contiguous uint8 tensor on a HIP device), without the EOF member, as a new uint8 tensor
    on the same device.  Runs on the current stream of that device and waits for it (the size of the result comes back)."""
    import torch
    if t.dtype != torch.uint8 or t.device.type != "cuda":
        raise ValueError("bgzf.compress: a uint8 tensor on a HIP device is expected")
    t = t.contiguous().view(-1)
    lib = _abi.load_library()
    n = t.numel()
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        dst = torch.empty(max(1, int(lib.vgl_bgzf_bound(n))), dtype=torch.uint8, device=t.device)
        ws_bytes = int(lib.vgl_bgzf_workspace_bytes(n))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=t.device)
        out_n = torch.zeros(1, dtype=torch.int64, device=t.device)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_bgzf_compress_device(dev, C.c_void_p(t.data_ptr()), n, C.c_void_p(dst.data_ptr()), dst.numel(), C.c_void_p(out_n.data_ptr()),
                                          C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != _abi.VGL_OK:
            raise RuntimeError(f"vgl_bgzf_compress_device: {lib.vgl_last_error().decode()} (code {rc})")
        total = int(out_n.item())
        return dst[:total].clone()


def write_file(path, pieces):
    """write compressed pieces (device tensors, host tensors or bytes) in order, then EOF"""
    with open(path, "wb") as f:
        for p in pieces:
            f.write(p if isinstance(p, (bytes, bytearray)) else p.cpu().numpy().tobytes())
        f.write(EOF)


class BgzfArgError(ValueError):
    """VGL_E_ARG from the library: a range outside the buffers, refused before the decoder ran"""


def index(raw):
    """the members of the BGZF stream `raw` (bytes): int64 begin, int32 csize and int32 isize arrays, the EOF member included.
    ValueError when the bytes are not a clean series of BGZF members (plain gzip, plain text, a cut member, trailing bytes)."""
    lib = _abi.load_library()
    raw = bytes(raw)
    buf = (C.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0")
    cap = len(raw) // 28 + 1
    begin, csize, isize = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n = C.c_int64()
    rc = lib.vgl_bgzf_index(buf, len(raw), cap, begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(n))
    if rc != _abi.VGL_OK:
        raise ValueError(f"vgl_bgzf_index: {lib.vgl_last_error().decode()} (code {rc})")
    return begin[:n.value].copy(), csize[:n.value].copy(), isize[:n.value].copy()


def inflate_members(src, begin, csize, out_off, isize, dst):
    """vgl_inflate_members_device on tensors of one device: src and dst uint8, begin and out_off int64, csize and isize int32.
    Returns the int32 status tensor (0: inflated, 1: left to the caller); BgzfArgError when a range lies outside the buffers."""
    import torch
    lib = _abi.load_library()
    dev = src.device.index if src.device.index is not None else torch.cuda.current_device()
    n = begin.numel()
    for t, dt in ((src, torch.uint8), (dst, torch.uint8), (begin, torch.int64), (out_off, torch.int64), (csize, torch.int32), (isize, torch.int32)):
        if t.dtype != dt or t.device.type != "cuda" or not t.is_contiguous():
            raise ValueError("bgzf.inflate_members: contiguous tensors on a HIP device are expected (uint8, int64 offsets, int32 sizes)")
    if not (csize.numel() == out_off.numel() == isize.numel() == n):
        raise ValueError("bgzf.inflate_members: one entry per member in every array")
    with torch.cuda.device(dev):
        status = torch.full((max(1, n),), -1, dtype=torch.int32, device=src.device)
        ws_bytes = int(lib.vgl_inflate_workspace_bytes(n))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=src.device)
        stream = torch.cuda.current_stream(dev)
        rc = lib.vgl_inflate_members_device(dev, C.c_void_p(src.data_ptr()), src.numel(), n, C.c_void_p(begin.data_ptr()), C.c_void_p(csize.data_ptr()),
                                            C.c_void_p(out_off.data_ptr()), C.c_void_p(isize.data_ptr()), C.c_void_p(dst.data_ptr()), dst.numel(),
                                            C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc == _abi.VGL_E_ARG:
            raise BgzfArgError(f"vgl_inflate_members_device: {lib.vgl_last_error().decode()} (code {rc})")
        if rc != _abi.VGL_OK:
            raise RuntimeError(f"vgl_inflate_members_device: {lib.vgl_last_error().decode()} (code {rc})")
        stream.synchronize()
        return status[:n]


def decompress(t):
    """the bytes a BGZF stream inflates to: `t` is a contiguous uint8 tensor on a HIP device holding whole members (an EOF member or
    none).  Returns (out, status) on the same device: out is the members' outputs back to back (ISIZE bytes each), status one int32
    per member -- _abi.INFLATE_OK, or _abi.INFLATE_HOST for a member the device did not take to its exact end (ISIZE bytes, CRC32,
    the data ending at the trailer), whose bytes in `out` are unspecified.  The counterpart of compress(t); runs on the current
    stream of that device and waits for it.  ValueError when the bytes are not a series of BGZF members."""
    import torch
    if t.dtype != torch.uint8 or t.device.type != "cuda":
        raise ValueError("bgzf.decompress: a uint8 tensor on a HIP device is expected")
    t = t.contiguous().view(-1)
    begin, csize, isize = index(t.cpu().numpy().tobytes())
    out_off = np.concatenate([[0], np.cumsum(isize, dtype=np.int64)])
    dst = torch.empty(max(1, int(out_off[-1])), dtype=torch.uint8, device=t.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(t.device)
    status = inflate_members(t, up(begin), up(csize), up(out_off[:-1]), up(isize), dst)
    return dst[:int(out_off[-1])], status
