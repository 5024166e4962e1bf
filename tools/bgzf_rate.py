#!/usr/bin/env python3
"""Rate of the device BGZF compressor (vcfgl_amd.bgzf) on a large buffer of VCF-like text: GL triples, depths and genotypes of
random samples, so that the data holds the short repeats program output holds.  Prints GB/s of input (device time between
events, fastest of the repeats) and the compression ratio; under `rocprofv3 --kernel-trace --stats -- python tools/bgzf_rate.py`
the per-kernel times come from the trace.
usage (GPU box): python tools/bgzf_rate.py [MB of input, default 1024] [repeats, default 3]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vcfgl_amd import bgzf  # noqa: E402

mb = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rng = np.random.default_rng(1)
gl = ["-0.30103", "-1.2041", "-4.78903", "-39.052", "-36.9795", "-2.7166", "0", "-0.60206"]
tok = [f"{a}/{b}:{d}:{gl[x]},{gl[y]},{gl[z]}" for a in "01" for b in "01" for d in range(1, 31) for x, y, z in ((0, 1, 3), (2, 0, 4), (3, 5, 0), (6, 7, 2))]
line = "\t".join(tok[i] for i in rng.integers(0, len(tok), 4000)).encode() + b"\n"
chunk = np.frombuffer(line * max(1, (64 << 20) // len(line)), dtype=np.uint8)
host = np.resize(chunk, mb << 20)
# vary the copies a little, so that the buffer is not 1 GB of one repeated 64 MB block
host[::4099] = rng.integers(48, 58, host[::4099].shape[0], dtype=np.uint8)
src = torch.from_numpy(host).to("cuda")
torch.cuda.synchronize()
best, out = None, None
for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = bgzf.compress(src)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    best = ms if best is None else min(best, ms)
print(f"bgzf on the device: {src.numel() / 1e9:.3f} GB in {best:.2f} ms (incl. allocation and the size read-back) = {src.numel() / best / 1e6:.1f} GB/s; "
      f"ratio {src.numel() / out.numel():.2f}")
