#!/usr/bin/env python3
"""Host model of the float32 pool loop's dealing (vgl_sample.hip, `if constexpr (F32)`): how many iterations a wavefront needs for its items
and how many lanes hold an item in an iteration, for the loop of VGL_POOL_ATTEMPTS 2 (attempt A, attempt B when A is rejected, one
gamma step), for the two half-steps of VGL_POOL_HALVES (attempt + gamma step, then the next attempt + gamma step where float32 settles
both without a bounded test) and for the carried lanes of VGL_POOL_CARRY (a lane whose item half-step 1 finished runs half-step 2 on the item
it claimed ahead).  No GPU: the loop's decisions are replaced by their measured frequencies.

What is modelled: 4 groups of 16 lanes, each dealing a quarter of the wavefront's items from a counter of its own (a lane holds its item and
one claimed ahead); an item = two gamma deviates; a normal attempt is accepted with probability 0.7303, 1.2 % of the attempts fall into the
logarithm test's band; a gamma step on an accepted attempt is not `sure` for G_AMB of them and accepted overall with probability 0.997
(first deviate) / 0.99997 (second); both bounded tests run every PERIOD-th iteration, a lane that needs one holds until then; an attempt
that is looked at again (after a hold, or left alone by attempt B / half-step 2) is the same attempt with the same outcome.

What is not: the Poisson spread of a wavefront's item count (1250 +- 35 at depth 20), deferred reads (1 in 10^4).

The stamped hooks build (tools/stamps.py 2 <depth>) measures the same three figures; the model is to reproduce those of the loop that
exists within a few percent before its figure for another loop is quoted:
    depth 20, VGL_POOL_ATTEMPTS 2: 46.71 iterations, 59.04 lanes with an item, 2.206 lane-iterations per item (profiles/r06_ab/stamps_lean2_depth20.txt)
    depth 20, two half-steps:      34.98 iterations, 56.76 lanes with an item, 1.589 lane-iterations per item (profiles/pool_halves_ab/stamps_lean2_depth20.txt)
    depth 20, carried lanes:       31.86 iterations, 56.30 lanes with an item, 1.435 lane-iterations per item, 18.1 lanes carried (profiles/pool_carry_ab/stamps_lean2_depth20.txt)
    depth 30: 69.89 / 59.19 / 2.206, 50.61 / 58.85 / 1.588 and 45.80 / 58.54 / 1.430 (stamps_lean2_depth30.txt in the same three directories)
(tests/test_pool_dealing_model_cpu.py holds the model to 4 % of these.)

usage: python tools/pool_dealing_model.py [wavefronts per case = 300] [seed = 1]"""
import random
import sys

GROUPS, LANES = 4, 64
P_ACC, P_AMB, P_AMB_ACC = 0.7303, 0.012, 0.5            # normal attempt: accepted overall; inside the band; accepted by the logarithm test
G_ACC = (0.997, 0.99997)                                # gamma step accepted, by stage
G_AMB = (0.0045, 0.0005)                                # gamma step not `sure`, by stage (0.25 % of the gamma steps: the stamped build's gamma-test blocks)
PERIOD = 4


def draw_attempt(rng, stage):
    """(normal, gamma): normal in acc / rej / amb_acc / amb_rej; gamma in sure / amb_acc / amb_rej (looked at only behind an accepted normal attempt)"""
    u = rng.random()
    if u < P_AMB:
        n = "amb_acc" if rng.random() < P_AMB_ACC else "amb_rej"
    else:
        n = "acc" if u < P_AMB + (P_ACC - P_AMB * P_AMB_ACC) else "rej"
    g = "sure"
    if rng.random() < G_AMB[stage]:
        g = "amb_rej" if rng.random() < (1.0 - G_ACC[stage]) / G_AMB[stage] else "amb_acc"
    return n, g


class Lane:
    def __init__(self):
        self.have, self.stage, self.pending = False, 0, []
        self.next_ok = self.carried = False         # the item claimed ahead exists; half-step 2 of this iteration ran on it

    def attempt(self, rng, i):
        """the i-th attempt from the lane's state (kept until consumed: a held or deferred attempt comes out the same)"""
        while len(self.pending) <= i:
            self.pending.append(draw_attempt(rng, self.stage))
        return self.pending[i]

    def consume(self, n, accepted):
        del self.pending[:n]
        if accepted:
            self.stage += 1
            self.pending = []               # (the next stage's attempts have that stage's gamma frequencies)


def gamma_step(lane, g, full):
    """-> (held, accepted)"""
    if g != "sure" and not full:
        return True, False
    return False, g != "amb_rej"


def step_attempts(lane, rng, full):
    n, g = lane.attempt(rng, 0)
    if n.startswith("amb") and not full:
        return True
    if n in ("acc", "amb_acc"):
        held, acc = gamma_step(lane, g, full)
        if not held:
            lane.consume(1, acc)
        return held
    nb, gb = lane.attempt(rng, 1)                       # A rejected: attempt B
    if nb == "acc":
        held, acc = gamma_step(lane, gb, full)
        if not held:
            lane.consume(2, acc)
        return held                                     # (held: nothing moves, A is looked at again)
    lane.consume(2 if nb == "rej" else 1, False)        # B inside the band: the next iteration's attempt A
    return False


def step_halves(lane, rng, full):
    n, g = lane.attempt(rng, 0)
    if n.startswith("amb") and not full:
        return True
    if n in ("acc", "amb_acc"):
        held, acc = gamma_step(lane, g, full)
        if held:
            return True
        lane.consume(1, acc)
    else:
        lane.consume(1, False)
    if lane.stage == 2:
        return False
    n, g = lane.attempt(rng, 0)                         # half-step 2: only what needs no bounded test
    if n == "rej":
        lane.consume(1, False)
    elif n == "acc" and g == "sure":
        lane.consume(1, True)
    return False


def step_carry(lane, rng, full):
    n, g = lane.attempt(rng, 0)
    if n.startswith("amb") and not full:
        return True
    if n in ("acc", "amb_acc"):
        held, acc = gamma_step(lane, g, full)
        if held:
            return True
        lane.consume(1, acc)
    else:
        lane.consume(1, False)
    if lane.stage == 2:
        if not lane.next_ok:
            return False
        lane.stage, lane.pending, lane.carried = 0, [], True        # the next item from its start state
    n, g = lane.attempt(rng, 0)                         # half-step 2 as in step_halves, on the lane's item or on the next one
    if n == "rej":
        lane.consume(1, False)
    elif n == "acc" and g == "sure":
        lane.consume(1, True)
    return False


def wavefront(items, step, rng):
    """-> (iterations, lane-iterations with an item, held lane-iterations, carried lane-iterations)"""
    per = LANES // GROUPS
    quarter = (items + GROUPS - 1) // GROUPS
    lanes = [Lane() for _ in range(LANES)]
    k, kn, ctr, end = [0] * LANES, [0] * LANES, [0] * GROUPS, [0] * GROUPS
    for g in range(GROUPS):
        beg = g * quarter
        end[g] = min(beg + quarter, items)
        ctr[g] = beg + 2 * per
        for j in range(per):
            ln = g * per + j
            k[ln], kn[ln] = beg + j, beg + j + per
            lanes[ln].have = k[ln] < end[g]
    iters = lane_iters = holds = carried = 0
    cnt = PERIOD
    while any(l.have for l in lanes):
        iters += 1
        cnt -= 1
        full = cnt == 0
        if full:
            cnt = PERIOD
        for ln, l in enumerate(lanes):
            if not l.have:
                continue
            lane_iters += 1
            l.next_ok = kn[ln] < end[ln // per]
            holds += step(l, rng, full)
            if l.stage == 2 or l.carried:               # finished: adopt the item claimed ahead, claim the next one of the group
                g = ln // per
                if l.carried:                           # (a carried lane keeps what half-step 2 left for that item)
                    carried += 1
                    l.carried = False
                else:
                    l.stage, l.pending = 0, []
                k[ln], kn[ln] = kn[ln], ctr[g]
                ctr[g] += 1
                l.have = k[ln] < end[g]
    return iters, lane_iters, holds, carried


LOOPS = (("attempts A / B", step_attempts), ("two half-steps", step_halves), ("carried lanes", step_carry))


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print(f"{waves} wavefronts per case, {GROUPS} groups of {LANES // GROUPS} lanes, period {PERIOD}")
    print(f"{'depth':>5} {'items':>6} {'loop':<16} {'iterations':>10} {'lanes with an item':>19} {'lane-iterations per item':>25} {'lanes holding':>14} {'lanes carried':>14}")
    for depth, items in ((20, 1250), (30, 1875)):
        res = {}
        for name, step in LOOPS:
            rng = random.Random(seed)
            tot = [0, 0, 0, 0]
            for _ in range(waves):
                for i, v in enumerate(wavefront(items, step, rng)):
                    tot[i] += v
            res[name] = tot[0] / waves
            print(f"{depth:>5} {items:>6} {name:<16} {tot[0] / waves:>10.2f} {tot[1] / tot[0]:>19.2f} {tot[1] / (waves * items):>25.3f} {tot[2] / tot[0]:>14.2f} {tot[3] / tot[0]:>14.2f}")
        print(f"{'':>5} {'':>6} iterations, two half-steps / attempts A / B: {res['two half-steps'] / res['attempts A / B']:.3f}, "
              f"carried lanes / two half-steps: {res['carried lanes'] / res['two half-steps']:.3f}")


if __name__ == "__main__":
    main()
