"""BGZF compression on the device (libvcfgl_hip.so, ABI 7: vgl_bgzf_compress_device).

What a rank of a sharded job uses for per-rank compressed output: each rank compresses its own bytes on its own GPU, and since
BGZF members are independent gzip members, the ranks' pieces concatenated in rank order (plus one EOF member) are a valid file.
Every piece but the last must hold a whole number of 0xff00-byte members' worth of input for the file to be the one a single
call would give; any split decompresses to the same bytes.

    pieces = [bgzf.compress(t) for t in chunks]     # device uint8 tensors in, device uint8 tensors out
    bgzf.write_file(path, pieces)                    # pieces + EOF
"""
import ctypes as C

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
