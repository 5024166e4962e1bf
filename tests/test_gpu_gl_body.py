"""The body of the GL kernels and the read-derived tags against tests/gl_body_model.py -- the likelihood from its definition, the
reference's float32 recurrence, GL model 1's published model, the counts and sums -- on the reads each tile drew.  Nothing here reads
the oracle: a term formula, a table row, a genotype index or the treatment of the unobserved allele that were wrong in the oracle and
the kernels alike would pass every parity test and fail here.

Cases: the table of test_gpu_gl_tail.py (gl_cases.PATHS: k_gl<4 | 5, 2>, k_gl<., 1>, both --precise-gl 1 cases, score 0, depth 40,
k_gl2, k_gl_redo, k_gl2 as shipped, both fused builds; both layouts, N = 1 / 63 / 65 / 130, 7 ... 33 sites) and gl_cases.BODY_EXTRA:
--error-qs 1, --adjust-qs 1 with --qs-bins, -doUnobserved 0 ... 5, depth 400 at N = 5, and -addQS 1 -addI16 1 with all AD tags at
N = 130.  Each case asserts from vgl_ctx_info() which build ran.

The dump.  Every case makes two calls on its context with the same flags, seed, site0 and genotypes: the first asks for the tags alone
-- the build under test, as a record loop runs it: asking for `reads` takes a fused context off the fused kernel and selects the
sampler's inline build --, the second for `reads` / `read_errp` as well.  In tile mode the reads of a (seed, site, sample) depend on
nothing else; fmt_dp, site_status, n_alleles and alleles2acgt of the two calls are asserted equal before anything is compared, and
read_capacity (the context's staging capacity) is asserted to hold the tile's largest depth, so no evaluation is left out.

Per case (gl_cases.check_body):
  * every live GL within the derived bound of gl2_exact (gl_body_model.py's docstring), every -inf and every missing value exactly
    where the model has it;
  * 0 values not identical to gl2_replay for table and fixed-score builds; --precise-gl 1: at most a share of 1e-5, each by one unit
    in the last place;
  * k_gl-model1: -10 GL within the tolerance test_oracle_errmod_model.py holds the same model to (rtol 2e-6, atol 1e-4 on each cost);
  * DP, AD, ADF + ADR, INFO/DP and INFO/AD equal to counts_from_reads in every case (from the call with the dump, where the call
    under test was not asked for them: FORMAT/AD would take a k_gl2 tile to k_gl); in the counts case all of them, I16 fields
    1-12 and QS (within N 2^-24 exact + 2^-149) from the call under test;
  * what the case must produce: its allele counts, -inf next to 0, an evaluation beyond 255 reads, samples without reads.
Each case prints the number of values, the largest depth, the worst ratio to the bound and the non-identical count."""
import pytest

import gl_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,sm,N", K.BODY_CASES, ids=K.case_ids(K.BODY_CASES))
def test_gl_and_read_sums_are_what_the_reads_define(name, sm, N, monkeypatch):
    entry = K.BODY_TABLE[name]
    sim, args, info = K.open_case(entry, name, sm, N, monkeypatch)
    _, gt = K.case_sites(entry, N)
    t = sim.simulate(3, gt, fields=K.case_fields(entry))
    dump = sim.simulate(3, gt, fields=K.DUMP_FIELDS, read_capacity=info["read_cap"], deviates=args.error_qs == 2)
    sim.close()
    assert info["read_cap"] >= int(t.numpy("fmt_dp").max(initial=0))
    msg, _, _ = K.check_body(name, entry, args, N, sm, t, dump)
    print(f"build: fused {info['fused']}, gl_wpb {info['gl_wpb']}, hooks {info['test_hooks']}, k_sample build {info['sample_lean']}")
