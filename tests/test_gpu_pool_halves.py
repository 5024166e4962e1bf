"""The float32 pool loop of the default tag surface (k_sample_seg<., ., 2> and k_sample<2, false, ., false, 2>) runs two attempt-and-gamma
half-steps per iteration: half-step 1 is a normal attempt with its gamma step, both bounded tests and every source of a deferred read;
half-step 2 takes the next attempt from the state and stage the first one left, and commits it only where float32 settles it without a
bounded test.  Every decision is the reference's, and every item's stream is addressed by (owner, read), so each case below must be
bit-equal to the oracle.  The shapes are the smallest at which each way the loop can go wrong shows: at most 16 sites each."""
import pytest

import synth
from test_gpu_parity import assert_parity, run_both
from vcfgl_amd import Simulator, VcfglArgs, _abi

pytestmark = pytest.mark.gpu

RTA3 = [(0, 2, 2), (3, 14, 12), (15, 30, 23), (31, 40, 37)]          # the rta3 bins (doc/error_qs.MD)


def args_of(depth, seed=23, beta_variance=1e-5, **kw):
    return VcfglArgs(seed=seed, depth=depth, error_rate=0.01, error_qs=2, beta_variance=beta_variance, add_pl=1, **kw)


def check(oracle, args, N, n_sites, hooks=False):
    assert n_sites <= 16
    want, got = run_both(oracle, args, synth.binary_sites(0, n_sites, N), hooks=hooks)
    assert_parity(want, got, check_gp=False)


def runs_the_float32_loop(args, N, hooks=False):
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    sim = Simulator(args, N, device=0, max_sites_per_tile=16, hooks=hooks)
    lean = sim.info()["sample_lean"]
    sim.close()
    return lean == 2


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_fewer_items_than_lanes(oracle, depth, N):
    """wavefronts with fewer items than lanes (most lanes never have one, the groups' quarters are ragged or empty), reads that the
    iteration which adopted them finishes, a second wavefront of one evaluation"""
    args = args_of(depth)
    assert runs_the_float32_loop(args, N)
    check(oracle, args, N, 16)


@pytest.mark.parametrize("depth,N,bins", [(20, 300, False), (20, 1000, False), (30, 130, True)])
def test_ordinary_pools_and_the_ragged_sixteenth_wavefront(oracle, depth, N, bins):
    """one segment per wavefront at the bench depths; 1000 samples: sixteen wavefronts per site, the last one with 40 evaluations; depth 30
    with --qs-bins (the finish block's table lookup)"""
    args = args_of(depth, **(dict(qs_bins=RTA3) if bins else {}))
    assert runs_the_float32_loop(args, N)
    check(oracle, args, N, 12)


@pytest.mark.parametrize("every,cap", [(3, None), (5, None), (7, None), (3, 16)])
def test_candidates_met_in_half_step_one_and_deferred_from_half_step_two(oracle, monkeypatch, every, cap):
    """VGL_DEBUG_REDO_EVERY sends every k-th candidate of the bounded tests (half-step 1 only) and of the finish block to k_redo; an attempt
    half-step 2 leaves alone meets its test as the next iteration's half-step 1.  cap 16: the list overflows into the bitmap."""
    monkeypatch.setenv("VGL_DEBUG_REDO_EVERY", str(every))
    if cap is not None:
        monkeypatch.setenv("VGL_DEBUG_REDO_CAP", str(cap))
    check(oracle, args_of(20, seed=77), 300, 10, hooks=True)


@pytest.mark.parametrize("period,period_n", [(1, 4), (3, 8), (4, 1), (8, 3)])
def test_holds_across_both_halves(oracle, monkeypatch, period, period_n):
    """a held lane moves in neither half; period 1: no lane is ever held, every iteration runs both bounded tests"""
    monkeypatch.setenv("VGL_SLOW_PERIOD", str(period))
    monkeypatch.setenv("VGL_SLOW_PERIOD_N", str(period_n))
    check(oracle, args_of(25, seed=19), 200, 16, hooks=True)


@pytest.mark.parametrize("pool,limit", [(64, None), (640, None), (None, 1)])
def test_segment_loop_and_list_kernel(oracle, monkeypatch, pool, limit):
    """the same loop inside the segment loop (k_sample<2, false, ., false, 2>: pools of 64 and 640 items, several segments per wavefront)
    and in the list kernel (k_sample_seg<., 2, 2>: every wavefront listed)"""
    if pool is not None:
        monkeypatch.setenv("VGL_DEBUG_POOL_CAP", str(pool))
        monkeypatch.setenv("VGL_SEG_SPLIT", "1")
    if limit is not None:
        monkeypatch.setenv("VGL_DEBUG_SEG_LIMIT", str(limit))
    check(oracle, args_of(20, seed=91), 300, 12, hooks=True)


def test_strand_and_quality_sum_build(oracle):
    """-addQS / -addI16 without --adjust-qs (k_sample_seg<., ., 4>) runs the two half-steps as well: the finishing lane also hands the score to the
    owner's quality sums.  (--adjust-qs runs k_sample_seg<., ., 3>, which keeps the loop of two attempts and one gamma step.)"""
    args = args_of(20, seed=31, add_qs=1, add_i16=1)
    args.rng_mode, args.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    gt = synth.acgt_sites(12, 300, seed=20, missing=0.03)
    sim = Simulator(args, 300, device=0, max_sites_per_tile=12)
    assert sim.info()["sample_lean"] == 3                  # (the deferred optional-tag builds, LEAN 3 and 4, report 3)
    got = sim.simulate(0, gt)
    sim.close()
    want = oracle.Oracle(args, 300).simulate(0, gt, fields=sim.default_fields())
    assert_parity(want, got, i16=True, check_gp=False)


@pytest.mark.parametrize("beta_variance", [1.2283e-5, 1e-9])
def test_beta_shapes(oracle, beta_variance):
    """--beta-variance 1.2283e-5: the smaller shape parameter is 0.01 (0.0099 / 1.2283e-5 - 1) = 8.05, just above the deferred builds' limit
    of 8, where w = 1 + a2 x < 0.5 (out of range) is most frequent in both halves; 1e-9: shape parameters of 1e5 and 1e7 (the sure-accept
    bound carries a slack that grows with them)"""
    args = args_of(20, seed=9, beta_variance=beta_variance)
    assert runs_the_float32_loop(args, 200)
    check(oracle, args, 200, 12)
