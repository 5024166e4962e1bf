"""Carried lanes of the float32 pool loop (VGL_POOL_CARRY, vgl_sample.hip): a lane whose item half-step 1 ended -- finished, or handed to
k_redo -- and that owns an item claimed ahead runs half-step 2 on that item, from the start state the finish block would have set.  An
item's stream is addressed by (owner, read) and half-step 2 commits only what needs no bounded test, so every item meets the same attempts
with the same decisions and each case below must be bit-equal to the oracle.  The shapes are the smallest at which each way the carry can
go wrong shows: at most 16 sites each."""
import pytest

import synth
from test_gpu_parity import assert_parity, run_both
from vcfgl_amd import Simulator, VcfglArgs, _abi

pytestmark = pytest.mark.gpu

RTA3 = [(0, 2, 2), (3, 14, 12), (15, 30, 23), (31, 40, 37)]          # the rta3 bins (doc/error_qs.MD)


def args_of(depth, seed=29, beta_variance=1e-5, **kw):
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
def test_no_next_item(oracle, depth, N):
    """about 64 (depth 1) or 128 (depth 2) items per wavefront, 16 or 32 per group of 16 lanes: few lanes or none own an item claimed ahead
    that exists -- the carry is all but never taken, and what the prefetch of a claim past the group's items read must stay unused"""
    args = args_of(depth)
    assert runs_the_float32_loop(args, N)
    check(oracle, args, N, 16)


@pytest.mark.parametrize("depth", [2, 3, 5])
def test_the_item_claimed_ahead_is_the_last(oracle, depth):
    """64 evaluations, 128 to 320 items in ragged quarters: some lanes of a group own a next item and others none; a lane that carries into
    its last item claims past the group's end"""
    args = args_of(depth, seed=41)
    assert runs_the_float32_loop(args, 64)
    check(oracle, args, 64, 16)


@pytest.mark.parametrize("depth,N,bins", [(20, 300, False), (20, 1000, False), (30, 130, True)])
def test_ordinary_pools(oracle, depth, N, bins):
    """one segment per wavefront at the bench depths; 1000 samples: the sixteenth wavefront has 40 evaluations; depth 30 with --qs-bins"""
    args = args_of(depth, **(dict(qs_bins=RTA3) if bins else {}))
    assert runs_the_float32_loop(args, N)
    check(oracle, args, N, 12)


@pytest.mark.parametrize("every,cap", [(3, None), (5, None), (7, None), (3, 16)])
def test_finish_by_redo_then_carry(oracle, monkeypatch, every, cap):
    """VGL_DEBUG_REDO_EVERY hands every k-th candidate of half-step 1's bounded tests and of the finish block to k_redo: the read sent
    there is the lane's item, the progress half-step 2 makes belongs to the item claimed ahead.  cap 16: the list overflows into the bitmap."""
    monkeypatch.setenv("VGL_DEBUG_REDO_EVERY", str(every))
    if cap is not None:
        monkeypatch.setenv("VGL_DEBUG_REDO_CAP", str(cap))
    check(oracle, args_of(20, seed=83), 300, 10, hooks=True)


@pytest.mark.parametrize("period,period_n", [(1, 4), (4, 1), (8, 3)])
def test_a_held_lane_neither_finishes_nor_carries(oracle, monkeypatch, period, period_n):
    monkeypatch.setenv("VGL_SLOW_PERIOD", str(period))
    monkeypatch.setenv("VGL_SLOW_PERIOD_N", str(period_n))
    check(oracle, args_of(25, seed=17), 200, 16, hooks=True)


@pytest.mark.parametrize("pool,limit", [(64, None), (640, None), (None, 1)])
def test_segment_loop_and_list_kernel(oracle, monkeypatch, pool, limit):
    """the same loop inside the segment loop (pools of 64 and 640 items) and in the list kernel (every wavefront listed): a segment's last
    items have no successor inside the segment"""
    if pool is not None:
        monkeypatch.setenv("VGL_DEBUG_POOL_CAP", str(pool))
        monkeypatch.setenv("VGL_SEG_SPLIT", "1")
    if limit is not None:
        monkeypatch.setenv("VGL_DEBUG_SEG_LIMIT", str(limit))
    check(oracle, args_of(20, seed=97), 300, 12, hooks=True)


def test_strand_and_quality_sum_build(oracle):
    """-addQS / -addI16 (k_sample_seg<., ., 4>): the finish block credits the score to the owner and base of the FINISHED item while the
    lane's stream, stage and first deviate already belong to the next one"""
    args = args_of(20, seed=37, add_qs=1, add_i16=1)
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
    """shape parameters just above the deferred builds' limit of 8 (out-of-range attempts hand reads to k_redo in half-step 1, then carry) and
    of 1e5 / 1e7"""
    args = args_of(20, seed=11, beta_variance=beta_variance)
    assert runs_the_float32_loop(args, 200)
    check(oracle, args, 200, 12)
