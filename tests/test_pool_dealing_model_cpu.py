"""tools/pool_dealing_model.py replaces the float32 pool loop's decisions by their frequencies; its figures are quoted for loops that do not
exist yet, so they must agree with what the stamped hooks build counted (tools/stamps.py 2 <depth>) for every loop that does: the loop of
two attempts (profiles/r06_ab), the two half-steps (profiles/pool_halves_ab) and the carried lanes (profiles/pool_carry_ab).

Bound: 4 % on iterations per wavefront and on lane-iterations per item -- twice the largest deviation the model showed on the loops it
was fitted to (1.9 %, depth 20, two half-steps).  100 wavefronts per case: the mean of 100 wavefronts of ~35 iterations with a spread of
about one iteration each is good to 0.3 %."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pool_dealing_model as model  # noqa: E402

WAVES = 100
STAMPS = {"attempts A / B": "r06_ab", "two half-steps": "pool_halves_ab", "carried lanes": "pool_carry_ab"}
ITEMS = {20: 1250, 30: 1875}


@pytest.mark.parametrize("depth", sorted(ITEMS))
@pytest.mark.parametrize("name,step", model.LOOPS, ids=[n for n, _ in model.LOOPS])
def test_model_agrees_with_the_stamped_loop(name, step, depth):
    st = json.load(open(os.path.join(ROOT, "profiles", STAMPS[name], f"stamps_lean2_depth{depth}.json")))
    assert abs(st["pool items"] - ITEMS[depth]) < 0.01 * ITEMS[depth]
    rng = random.Random(1)
    iters = lane_iters = carried = 0
    for _ in range(WAVES):
        i, l, _h, c = model.wavefront(ITEMS[depth], step, rng)
        iters, lane_iters, carried = iters + i, lane_iters + l, carried + c
    got_it, got_li = iters / WAVES, lane_iters / (WAVES * ITEMS[depth])
    want_it, want_li = st["pool iterations"], st["lanes with an item"] / st["pool items"]
    print(f"{name}, depth {depth}: iterations {got_it:.2f} (stamped {want_it:.2f}), lane-iterations per item {got_li:.3f} (stamped {want_li:.3f})")
    assert abs(got_it - want_it) <= 0.04 * want_it
    assert abs(got_li - want_li) <= 0.04 * want_li
    if name == "carried lanes":
        want_c = st["lanes carried"] / st["pool iterations"]
        print(f"  lanes carried per iteration {carried / iters:.2f} (stamped {want_c:.2f})")      # (shown, not bounded: the model was not fitted to it)
        assert carried > 0 and want_c > 0
    else:
        assert carried == 0
