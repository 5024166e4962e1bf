"""What tests/test_gpu_inflight.py is built from and what needs no GPU: the fixed sequences of big and small items, the byte
condition, and the tail-first check that makes a wait that returned too early visible.

A big item moves at least BIG_BYTES across the link (or writes them on the device); a small one is 1 site, line, member or byte;
a zero item (where the entry admits n = 0) is empty.  No link moves 64 MiB in under about a millisecond, a small item is done in
well under 100 microseconds -- a condition on bytes, asserted as such; no time is asserted anywhere.

The check: every destination is filled with POISON before its submit.  The first thing done after a wait returns is `tails()`: a
copy of the last TAIL bytes of what each destination should now hold (copies run front to back, so the tail is what a late copy has
not reached yet).  Only then is the whole compared.  `late()` names the destinations whose tail snapshot differs from the wanted
bytes and says whether the whole, read afterwards, is right by then (the signature of a premature return) or wrong too."""
import numpy as np

POISON = 0xA5
TAIL = 4096
BIG_BYTES = 64 << 20
PATTERN = "BssBBsBsz"          # big -> small, small -> small, small -> big, big -> big; z: an item of 0 sites where the entry admits one


def kinds(zero=True):
    """the sequence's kinds, in order: 'B', 's', and 'z' at the end where the entry admits an empty item"""
    return [k for k in PATTERN if zero or k != "z"]


def neighbours(seq):
    """the set of (kind, next kind) among 'B' and 's' items"""
    ks = [k for k in seq if k in "Bs"]
    return set(zip(ks, ks[1:]))


def big_count(unit_bytes):
    """the smallest count of units (sites, lines, members) of unit_bytes each that meets the byte condition"""
    assert unit_bytes > 0
    return -(-BIG_BYTES // int(unit_bytes))


class Item:
    def __init__(self, index, kind, n, first, seed):
        self.index, self.kind, self.n, self.first, self.seed = index, kind, n, first, seed

    def __repr__(self):
        return f"Item({self.index}, {self.kind!r}, n={self.n}, first={self.first}, seed={self.seed})"


def sequence(unit_bytes, seed, zero=True, first=0):
    """The items of one sequence: big items of big_count(unit_bytes) units, small ones of 1, zero ones of 0.  Item k covers the units
    [first_k, first_k + n_k) back to back (tile mode: absolute sites, so every item's content is distinct) and carries its own seed
    for content that is drawn.  Deterministic: nothing but the arguments goes in."""
    nbig = big_count(unit_bytes)
    out, at = [], int(first)
    for i, k in enumerate(kinds(zero)):
        n = {"B": nbig, "s": 1, "z": 0}[k]
        out.append(Item(i, k, n, at, int(seed) * 1000 + i))
        at += n
    return out


def sample_sites(n, count=8):
    """`count` sites of a tile of n: the first, the last and count - 2 evenly between them (all of them where n <= count)"""
    if n <= count:
        return list(range(n))
    return sorted({int(round(j * (n - 1) / (count - 1))) for j in range(count)})


def as_bytes(a):
    """a flat uint8 view of a C-contiguous array (float32 is thereby compared as bits)"""
    a = np.asarray(a)
    assert a.flags["C_CONTIGUOUS"]
    return a.reshape(-1).view(np.uint8)


def poison(*arrays):
    for a in arrays:
        as_bytes(a)[:] = POISON


def tails(dests):
    """{name: (copy of the last TAIL bytes of the first `used` bytes, used)} of dests = {name: (array, used bytes or None = all)} --
    call it first after a wait returns, before anything else reads the destinations"""
    out = {}
    for name, (a, used) in dests.items():
        b = as_bytes(a)
        used = b.size if used is None else int(used)
        out[name] = (b[max(0, used - TAIL):used].copy(), used)
    return out


def late(snapshot, dests, wants):
    """The findings, [] when there are none.  snapshot: what tails() returned; dests as for tails() (read now, whole); wants:
    {name: array of the wanted bytes}.  A destination whose tail was not there at the snapshot is reported whether or not the whole is
    right by now."""
    bad = []
    for name, (tail, used) in snapshot.items():
        want = as_bytes(wants[name])
        got = as_bytes(dests[name][0])[:used]
        if want.size != used:
            bad.append(f"{name}: {used} bytes delivered, {want.size} wanted")
            continue
        wt = want[max(0, used - TAIL):used]
        whole = np.array_equal(got, want)
        if not np.array_equal(tail, wt):
            at = int(np.flatnonzero(tail != wt)[0])
            pois = bool((tail[tail != wt] == POISON).all())
            bad.append(f"{name}: tail not there when the wait returned (first at byte {max(0, used - TAIL) + at} of {used}; "
                       f"{'still poison' if pois else 'other bytes'}); the whole is {'right' if whole else 'wrong'} when read afterwards")
        elif not whole:
            at = int(np.flatnonzero(got != want)[0])
            bad.append(f"{name}: differs at byte {at} of {used}")
    return bad


def untouched_behind(a, used):
    """what lies behind the first `used` bytes of a poisoned destination is still poison"""
    return bool((as_bytes(a)[int(used):] == POISON).all())
