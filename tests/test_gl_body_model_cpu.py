"""tests/gl_body_model.py -- GL model 2 from its definition, the reference's float32 recurrence, GL model 1, the read-derived counts
and sums -- against the CPU oracle in tile mode, at the cases and shapes of test_gpu_gl_body.py (planes layout; the counts case in
both).  No GPU.  The oracle returns the reads it drew (`reads`, `read_errp`), the model restates every GL and tag from them:

  * every GL within the derived bound of gl2_exact (the docstring of gl_body_model.py), -inf and missing exactly in place;
  * 0 values not identical to gl2_replay for table and fixed-score terms; --precise-gl 1: at most a share of 1e-5, each by one unit
    in the last place (DESIGN.md's float criterion);
  * DP, AD, ADF + ADR, INFO/DP and INFO/AD equal in every case; I16 fields 1-12 equal and QS within N 2^-24 exact + 2^-149 in the
    counts case;
  * the regenerated score table (seven significant digits of the exact term at 200 bits) equals the oracle's for scores 0 .. 92;
  * POWER: five deliberately wrong models each leave the bound on at least one case."""
import numpy as np
import pytest

import gl_body_model as B
import gl_cases as K
import gl_tail_model as M

CPU_CASES = [(n, sm, N) for n, sm, N in K.BODY_CASES if not sm or K.BODY_TABLE[n][4].get("counts")]


def oracle_case(oracle, name, sm, N):
    entry = K.BODY_TABLE[name]
    args = K.case_args(entry, sm)
    _, gt = K.case_sites(entry, N)
    o = oracle.Oracle(args, N)
    cap, dev = K.staging_capacity(args.depth), args.error_qs == 2
    t = o.simulate(3, gt, fields=K.case_fields(entry), read_capacity=cap, deviates=dev)
    dump = o.simulate(3, gt, fields=K.DUMP_FIELDS, read_capacity=cap, deviates=dev)      # (a second call, as on the device)
    o.close()
    return entry, args, t, dump


@pytest.mark.parametrize("name,sm,N", CPU_CASES, ids=K.case_ids(CPU_CASES))
def test_oracle_writes_what_the_model_states(oracle, name, sm, N):
    entry, args, t, dump = oracle_case(oracle, name, sm, N)
    K.check_body(name, entry, args, N, sm, t, dump)


def test_regenerated_score_table_equals_the_oracles(oracle):
    """3 x 93 entries: the exact term at 200 bits rounded to seven significant digits (the reference's literals agree with that for
    scores 0 .. 92 and differ in the last digit from 93 on; staged scores are six bits)"""
    tab = B.table(92)
    assert tab.shape == (3, 93)
    lib = oracle.lib()
    for row in range(3):
        for q in range(93):
            have, want = float(tab[row][q]), lib.vgl_oracle_q2gl(row, q)
            assert have == want, (row, q, have, want)
    assert tab[0][0] == -np.inf and np.all(np.isfinite(tab[1:, :])) and np.all(tab[:, 1:] < 0)


# the cases the mutants are tried on (N = 65, planes): the default build's flags, per-read scores, score 0, both --precise-gl 1 cases
POWER_CASES = ("k_gl-A5", "adjust-qs-bins", "k_gl-score-0", "precise", "precise-error-rate-0", "unobserved-4")


def test_wrong_models_leave_the_bound(oracle):
    """each mutant of gl2_exact -- e/3 in place of e/6 in the one-match term; the table row of score q + 1; the unobserved allele
    treated as allele 0 for matching; the maximum over the observed alleles' genotypes only; the two homozygous terms swapped -- is
    outside its own bound against the oracle (or puts a -inf where the oracle has none) on at least one case: a bound that could not
    tell them from the model would be too loose"""
    caught = {m: [] for m in B.MUTANTS}
    for name in POWER_CASES:
        entry, args, t, _ = oracle_case(oracle, name, 0, 65)
        mt = K.model_tile(t, args)
        gl = M.canon_bits(t, "gl", 0)
        x, bound, _ = B.gl2_exact(mt)
        _, worst, bad = B.compare_gl(gl, x, bound, mt.live)
        assert worst <= 1.0 and bad == 0
        for m in B.MUTANTS:
            try:
                xm, bm, _ = B.gl2_exact(mt, mutant=m)
            except AssertionError:                                   # (a score the mutant moves out of the table's range)
                continue
            _, wm, badm = B.compare_gl(gl, xm, bm, mt.live)
            print(f"{name}: mutant {m}: worst error / bound {wm:.3g}, misplaced {badm}")
            if wm > 1.0 or badm:
                caught[m].append(name)
    for m in B.MUTANTS:
        assert caught[m], f"mutant {m} is inside the bound on every case"
