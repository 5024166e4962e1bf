"""Writes tests/golden/ref_samplers.json: what the reference's own samplers and tables return (oracle/_ref, built by
`make -C oracle ref` where the reference checkout is present) for the inputs tests/test_oracle_vs_ref.py checks the oracle
on.  Every sequence is stored as its length, dtype, the sha256 of its little-endian bytes and its first values.

usage: python oracle/ref_vectors.py"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = os.path.join(ROOT, "oracle", "_ref", "libvgl_ref_stdbeta.so")
R48 = os.path.join(ROOT, "oracle", "_ref", "libvgl_ref_rand48beta.so")
OUT = os.path.join(ROOT, "tests", "golden", "ref_samplers.json")

# the inputs of tests/test_oracle_vs_ref.py
RAND48_SEEDS = [42, 0, -1, 123456789, -7, 2 ** 31 - 1]
RAND48_DRAWS = 2000
GAMMA_LN_X = (0.5, 700.0, 20000)           # np.linspace arguments
POISSON_LAMBDAS = [0, 0.1, 2, 5, 10, 11.99, 12, 20, 30, 100, 499.5]
BETA_MV = [(0.01, 1e-5), (0.024, 1e-5), (0.4, 0.1), (0.2, 0.1), (0.001, 1e-7)]
DRAWS = 20000
QS_TO_ERRPROB = list(range(0, 80))
HEAD = 32


def entry(a):
    a = np.ascontiguousarray(a)
    a = a.astype(a.dtype.newbyteorder("<"))
    return {"n": int(a.size), "dtype": a.dtype.str, "sha256": hashlib.sha256(a.tobytes()).hexdigest(), "head": a.ravel()[:HEAD].tolist()}


def _ref(path):
    r = C.CDLL(path)
    for f in ("ref_rng0", "ref_rng1", "ref_rng2", "ref_q2log10gl", "ref_qs_to_errprob"):
        getattr(r, f).restype = C.c_double
    r.ref_gamma_ln.restype = C.c_double
    r.ref_gamma_ln.argtypes = [C.c_double]
    r.ref_poisson.argtypes = [C.c_double, C.c_int, C.c_void_p]
    r.ref_beta.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    return r


def main():
    rs, rr = _ref(STD), _ref(R48)
    g = {"rand48": {}, "poisson": {}, "beta_std": {}, "beta_rand48": {}}
    for seed in RAND48_SEEDS:
        rs.ref_seed(seed)
        u = np.array([[rs.ref_rng0(), rs.ref_rng1(), rs.ref_rng2()] for _ in range(RAND48_DRAWS)])
        g["rand48"][str(seed)] = [entry(u[:, k]) for k in range(3)]
    g["gamma_ln"] = entry(np.array([rs.ref_gamma_ln(v) for v in np.linspace(*GAMMA_LN_X)]))
    g["q2log10gl"] = entry(np.array([[rs.ref_q2log10gl(row, q) for q in range(257)] for row in range(3)]))
    for lam in POISSON_LAMBDAS:
        a = np.zeros(DRAWS, np.int32)
        rs.ref_seed(42)
        rs.ref_poisson(lam, DRAWS, a.ctypes.data)
        g["poisson"][repr(lam)] = entry(a)
    for m, v in BETA_MV:
        a = np.zeros(DRAWS)
        rs.ref_beta(m, v, 42, DRAWS, a.ctypes.data)
        g["beta_std"][repr((m, v))] = entry(a)
        b = np.zeros(DRAWS)
        rr.ref_seed(42)
        rr.ref_beta(m, v, 42, DRAWS, b.ctypes.data)
        g["beta_rand48"][repr((m, v))] = entry(b)
    g["qs_to_errprob"] = entry(np.array([rs.ref_qs_to_errprob(q) for q in QS_TO_ERRPROB]))
    with open(OUT, "w") as f:
        json.dump(g, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
