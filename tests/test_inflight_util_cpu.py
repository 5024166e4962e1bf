"""tests/inflight_util.py without a GPU: the sequence generator (determinism, the neighbour kinds, the byte condition) and the
tail-first checker against a Python thread that fills a poisoned buffer late -- the late fill is reported, a fill in time is
accepted.  The thread is released by an event, not by a clock: nothing here sleeps."""
import threading

import numpy as np
import pytest

import inflight_util as iu


@pytest.mark.parametrize("unit", [1, 42013, 65280, 1 << 20, iu.BIG_BYTES, iu.BIG_BYTES + 1])
@pytest.mark.parametrize("zero", [True, False])
def test_sequence_is_fixed_and_meets_the_byte_condition(unit, zero):
    a, b = iu.sequence(unit, seed=5, zero=zero, first=17), iu.sequence(unit, seed=5, zero=zero, first=17)
    assert [vars(x) for x in a] == [vars(x) for x in b]
    assert 8 <= len(a) <= 10
    assert iu.neighbours(x.kind for x in a) >= {("B", "s"), ("s", "B"), ("B", "B")}
    assert ("z" in [x.kind for x in a]) == zero
    for x in a:
        if x.kind == "B":
            assert x.n * unit >= iu.BIG_BYTES > (x.n - 1) * unit           # the smallest count that meets it
        else:
            assert x.n == (1 if x.kind == "s" else 0)
    # back to back and distinct: no two items share a unit or a seed
    assert a[0].first == 17 and all(y.first == x.first + x.n for x, y in zip(a, a[1:]))
    assert len({x.seed for x in a}) == len(a)
    assert [vars(x) for x in iu.sequence(unit, seed=6, zero=zero, first=17)] != [vars(x) for x in a]


def test_sample_sites():
    assert iu.sample_sites(1) == [0] and iu.sample_sites(8) == list(range(8))
    for n in (9, 100, 1598, 4096):
        s = iu.sample_sites(n)
        assert len(s) == 8 and s[0] == 0 and s[-1] == n - 1 and s == sorted(set(s))


def filled_by_a_thread(n, used, want, release_before_snapshot):
    """a poisoned destination of n bytes that a thread fills front to back with `want` once it is released; the snapshot is taken
    before or after the release.  Returns late()'s findings."""
    dst = np.empty(n, dtype=np.uint8)
    iu.poison(dst)
    go = threading.Event()

    def fill():
        go.wait()
        for lo in range(0, used, 1 << 16):
            dst[lo:min(used, lo + (1 << 16))] = want[lo:min(used, lo + (1 << 16))]

    t = threading.Thread(target=fill)
    t.start()
    dests = {"dst": (dst, used)}
    if release_before_snapshot:
        go.set()
        t.join()
    snap = iu.tails(dests)                           # "the wait has returned"
    go.set()
    t.join()
    found = iu.late(snap, dests, {"dst": want})
    assert iu.untouched_behind(dst, used)
    return found


@pytest.mark.parametrize("n,used", [(1, 1), (100, 100), (iu.TAIL, iu.TAIL), (iu.TAIL + 1, iu.TAIL + 1), (1 << 20, (1 << 20) - 333)])
def test_a_late_fill_is_reported_and_a_fill_in_time_is_accepted(n, used):
    want = np.random.default_rng(n).integers(0, 256, used, dtype=np.uint8)
    want[-1] = iu.POISON ^ 0xFF                      # (the last byte is never the poison by chance)
    assert filled_by_a_thread(n, used, want, True) == []
    found = filled_by_a_thread(n, used, want, False)
    assert len(found) == 1 and "tail not there" in found[0] and "still poison" in found[0] and "the whole is right" in found[0]


def test_wrong_bytes_and_wrong_sizes_are_reported():
    want = np.arange(10000, dtype=np.uint32)
    got = want.copy()
    dests = {"x": (got, None)}
    assert iu.late(iu.tails(dests), dests, {"x": want}) == []
    got[5] ^= 1                                      # in the body: seen by the whole comparison only
    f = iu.late(iu.tails(dests), dests, {"x": want})
    assert len(f) == 1 and "differs at byte 20 of 40000" in f[0]
    got[5] ^= 1
    got[-1] ^= 1 << 24                               # in the tail: both readings are wrong
    f = iu.late(iu.tails(dests), dests, {"x": want})
    assert len(f) == 1 and "other bytes" in f[0] and "the whole is wrong" in f[0]
    f = iu.late(iu.tails({"x": (got, 36000)}), {"x": (got, 36000)}, {"x": want})
    assert len(f) == 1 and "36000 bytes delivered, 40000 wanted" in f[0]
    # float32 is compared as bits: -0.0 is not 0.0, a NaN equals itself
    a = np.array([0.0, np.nan], dtype=np.float32)
    b = np.array([-0.0, np.nan], dtype=np.float32)
    assert iu.late(iu.tails({"f": (a, None)}), {"f": (a, None)}, {"f": a.copy()}) == []
    assert iu.late(iu.tails({"f": (a, None)}), {"f": (a, None)}, {"f": b}) != []
