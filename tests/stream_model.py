"""numpy model of vgl_stream_assemble_device: a tile's heads and bodies interleaved site by site.

Both offset arrays are non-decreasing prefix sums that may start at any value; `heads` and `bodies` start at site 0's first byte."""
import numpy as np


def assemble(heads, head_offsets, bodies, body_offsets):
    """(stream, record_offsets): uint8 [total] and int64 [n_sites + 1], record i = head i then body i at record_offsets[i]"""
    heads = np.asarray(heads, dtype=np.uint8)
    bodies = np.asarray(bodies, dtype=np.uint8)
    ho = np.asarray(head_offsets, dtype=np.int64)
    bo = np.asarray(body_offsets, dtype=np.int64)
    assert ho.shape == bo.shape and ho.ndim == 1 and ho.size >= 1
    assert (np.diff(ho) >= 0).all() and (np.diff(bo) >= 0).all()
    ho, bo = ho - ho[0], bo - bo[0]
    rec = ho + bo
    out = np.empty(int(rec[-1]), dtype=np.uint8)
    for i in range(ho.size - 1):
        hl = int(ho[i + 1] - ho[i])
        out[rec[i]:rec[i] + hl] = heads[ho[i]:ho[i + 1]]
        out[rec[i] + hl:rec[i + 1]] = bodies[bo[i]:bo[i + 1]]
    return out, rec
