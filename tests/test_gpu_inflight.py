"""The asynchronous entry points with large, uneven work in flight (tests/inflight_util.py holds the sequences and the check).

Every sequence is `B s s B B s B s z`: big items (at least 64 MiB cross the link or are written on the device -- asserted as a
byte count; no time is asserted anywhere), items of one site / line / member / byte, and an empty item where the entry admits one.
Two items are in flight wherever the entry allows (item k + 1 is submitted before the wait for k).  Every destination is poisoned
before its submit, the last 4 KiB of each is read first when the wait returns, the whole afterwards, and the buffers of item k are
given to item k + 2 at once, as a record loop does.  Nothing is compared with the asynchronous path itself: (a) the same items one
at a time through the synchronous entry on a fresh context or handle, bytes for bytes (float32 as bits), and (b) an anchor that owes
nothing to the library -- the oracle on 8 sites of every big tile and on every small one, zlib, the families' CPU models.

`-s` prints every sequence's per-item wait times (to be read, not asserted)."""
import ctypes as C
import queue
import threading
import time
import zlib

import numpy as np
import pytest
import torch

import bcfin_cases as bc
import bcfin_model as bm
import bgzf_model
import inflate_corpus as ic
import inflight_util as iu
import stream_model as sm
import synth
import vcfin_cases as vc
from vcfgl_amd import Simulator, VcfglArgs, _abi, vcftext

pytestmark = pytest.mark.gpu
N = 500                                                      # samples of every tile (the workload's own shape has 1000)
PLANE_FIELDS = ["site_status", "n_alleles", "alleles2acgt", "fmt_dp", "gl", "pl"]
SITE_FIELDS = ["site_status", "n_alleles", "alleles2acgt", "fmt_dp"]
KIND = {name: (dtype, kind) for name, dtype, kind in _abi.TILE_FIELDS}
M = bgzf_model.MEMBER


def show(name, items, waits):
    print(f"\n{name}: wait per item (ms): " + " ".join(f"{it.kind}{it.n}:{1e3 * w:.2f}" for it, w in zip(items, waits)))


class Pinned:
    """page-locked host arrays (vgl_host_alloc), freed together; pageable=True: ordinary numpy memory with the same interface"""

    def __init__(self, lib, pageable=False):
        self.lib, self.ptrs, self.pageable = lib, [], pageable

    def array(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.pageable:
            return np.empty(max(n, 1), dtype=np.uint8)[:n].view(dtype).reshape(shape)
        p = self.lib.vgl_host_alloc(max(n, 1))
        assert p
        self.ptrs.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].view(dtype).reshape(shape)

    def close(self):
        for p in self.ptrs:
            self.lib.vgl_host_free(p)
        self.ptrs = []


def _shape(kind, n_sites, n_samples, A, G):
    """the shape of a vgl_tile_out array of n_sites sites (include/vcfgl_hip.h: per site, per (site, sample), per (site, k, sample))"""
    return {"site": (n_sites,), "site5": (n_sites, 5), "siteA": (n_sites, A), "site16": (n_sites, 16), "eval": (n_sites, n_samples),
            "planeG": (n_sites, G, n_samples), "planeA": (n_sites, A, n_samples)}[kind]


def field_site_bytes(f, A, G):
    dtype, kind = KIND[f]
    return int(np.prod(_shape(kind, 1, N, A, G))) * np.dtype(dtype).itemsize


class DestSet:
    """the caller's output arrays of one slot: a vgl_tile_out over `mem` arrays of cap sites"""

    def __init__(self, mem, fields, cap, A, G):
        self.fields, self.A, self.G = fields, A, G
        self.arr = {f: mem.array(_shape(KIND[f][1], cap, N, A, G), KIND[f][0]) for f in fields}
        self.struct = _abi.TileOut()
        for f, a in self.arr.items():
            setattr(self.struct, f, a.ctypes.data)
        iu.poison(*self.arr.values())

    def poison(self, n):
        """the first n sites again: with what lies behind them still poison (checked after every wait), the whole set is poison"""
        for a in self.arr.values():
            iu.poison(a[:n])

    def dests(self, n):
        return {f: (a, n * field_site_bytes(f, self.A, self.G)) for f, a in self.arr.items()}


def tile_args(**kw):
    base = dict(seed=42, depth=2, error_rate=0.01, error_qs=2, beta_variance=1e-5, add_pl=1)
    base.update(kw)
    mode = base.pop("rng_mode", _abi.VGL_RNG_TILE)
    layout = base.pop("out_layout", _abi.VGL_LAYOUT_PLANES)
    a = VcfglArgs(**base)
    a.rng_mode, a.out_layout = mode, layout
    a.beta_sampler = _abi.VGL_BETA_STD if mode == _abi.VGL_RNG_SERIAL else _abi.VGL_BETA_RAND48
    return a


def genotypes(items):
    return [np.ascontiguousarray(synth.binary_sites(it.first, it.n, N)) for it in items]


def one_at_a_time(args, items, gts, fields, hooks=False, tables=None):
    """(a): every item through vgl_simulate_tile on a fresh context, nothing else in flight; [{field: array of the item's sites}].
    tables: a list that receives every tile's own discordance table (vgl_ctx_discordance, read and reset after each tile)"""
    sim = Simulator(args, N, device=0, max_sites_per_tile=max(it.n for it in items), hooks=hooks)
    if tables is not None:
        sim.discordance(1)
    out = []
    for it, gt in zip(items, gts):
        t = sim.simulate(it.first, gt, fields=fields)
        out.append({f: t.numpy(f) for f in fields})
        if tables is not None:
            tables.append(sim.discordance_table(reset=True))
    sim.close()
    return out


def record_loop(items, submit, wait, after):
    """item k + 1 is submitted before the wait for k; after(k, rc) runs as the first thing when the wait for k has returned.
    Returns the wait times."""
    waits = []

    def finish(j):
        t0 = time.perf_counter()
        rc = wait(j)
        waits.append(time.perf_counter() - t0)
        after(j, rc)

    for k in range(len(items)):
        submit(k)
        if k > 0:
            finish(k - 1)
    finish(len(items) - 1)
    return waits


def undefined(args, f, n_alleles):
    """VGL_LAYOUT_SAMPLE_MAJOR: the positions of field f's slabs [n][G * N] that lie behind the records' arrays (a site of nA alleles
    holds N * nA (nA + 1) / 2 values; what lies behind them is unspecified); None where every position is a result"""
    if args.out_layout != _abi.VGL_LAYOUT_SAMPLE_MAJOR or KIND[f][1] != "planeG":
        return None
    nA = np.asarray(n_alleles, dtype=np.int64)
    return np.arange(args.max_genotypes * N)[None, :] >= (N * (nA * (nA + 1) // 2))[:, None]


def settled(args, want, dests):
    """`want` with the unspecified positions of its sample-major slabs taken as delivered: they are not results"""
    out = dict(want)
    for f in want:
        if f not in KIND:
            continue
        u = undefined(args, f, want["n_alleles"])
        if u is not None and u.any():
            n = u.shape[0]
            w = np.array(want[f]).reshape(n, -1)
            w[u] = dests[f][0][:n].reshape(n, -1)[u]
            out[f] = w
    return out


def against_the_oracle(oracle, args, items, gts, sync, fields):
    """(b) for tiles: the oracle on 8 sites of every big tile (first, last, six between) and on every small one.  In tile mode a value
    depends on (seed, absolute site, sample) only, so the oracle is called with the sampled site as site0"""
    orc = oracle.Oracle(args, N)
    for it, gt, got in zip(items, gts, sync):
        for s in iu.sample_sites(it.n):
            want = orc.simulate(it.first + s, gt[s:s + 1], fields=fields)
            for f in fields:
                w, g = want.numpy(f).reshape(1, -1), np.ascontiguousarray(got[f][s:s + 1]).reshape(1, -1)
                u = undefined(args, f, want.numpy("n_alleles"))
                if u is not None:
                    assert np.array_equal(want.numpy("n_alleles"), got["n_alleles"][s:s + 1])
                    w, g = w[~u], g[~u]
                assert np.array_equal(iu.as_bytes(np.ascontiguousarray(w)), iu.as_bytes(np.ascontiguousarray(g))), (it, s, f)
    orc.close()


# ---- 1. plain tiles ---------------------------------------------------------------------------------------------------------------------

def fetched_of(args, planes, a, b):
    """the stateless fetch-GL formatter (vgl_fetchgl_format_device) on host planes: (text as uint8, offsets int64)"""
    from vcfgl_amd import fetchgl
    n = planes["site_status"].shape[0]
    dev = {f: torch.from_numpy(np.ascontiguousarray(planes[f])).cuda() for f in ("site_status", "n_alleles", "alleles2acgt", "gl")}
    dst = torch.empty(fetchgl.bound(N, n), dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    fetchgl.format_into(dev["site_status"], dev["n_alleles"], dev["alleles2acgt"], dev["gl"], a, b, _abi.FETCHGL_FLOAT, dst, off,
                        max_genotypes=args.max_genotypes, layout=args.out_layout)
    torch.cuda.synchronize()
    off = off.cpu().numpy()
    return dst[:int(off[-1])].cpu().numpy(), off


def piled_of(args, it, gt, read_cap):
    """the stateless pileup formatter (vgl_pileup_format_device) on the planes and the read dump of the tile run alone on a fresh
    context with a host read dump of the context's staging capacity: (text as uint8, offsets int64)"""
    from vcfgl_amd import pileup
    sim = Simulator(args, N, device=0, max_sites_per_tile=it.n)
    assert sim.info()["read_cap"] == read_cap
    t = sim.simulate(it.first, gt, fields=["site_status", "fmt_dp"], read_capacity=read_cap)
    sim.close()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert 0 < int(t.numpy("fmt_dp").max()) <= read_cap
    text, off = pileup.format_columns(dev(t.numpy("site_status")), dev(t.numpy("fmt_dp")), dev(t.numpy("reads")), N)
    return text.cpu().numpy(), off.cpu().numpy()


class Side:
    """a text side output of the big tiles (vgl_ctx_fetchgl_next / vgl_ctx_pileup_next): a request per slot over page-locked, poisoned
    text and offsets, armed before a big tile's submit; want[k] = (text, offsets) of the stateless formatter"""

    def __init__(self, name, mem, struct, arm, cap, big, want):
        self.name, self.arm, self.want = name, arm, want
        self.text, self.off = [mem.array((cap,), np.uint8) for _ in range(2)], [mem.array((big + 1,), np.int64) for _ in range(2)]
        iu.poison(*self.text, *self.off)
        self.req = [struct(self.text[s].ctypes.data, cap, self.off[s].ctypes.data, -7) for s in range(2)]
        assert all(len(t) > 0 for t, _ in want.values())


def run_plain(oracle, name, args, fields, pageable=False, with_oracle=True, first=1000, disc=False, fetch=None, pile=False):
    lib = _abi.load_library()
    A, G = args.max_alleles, args.max_genotypes
    unit = sum(field_site_bytes(f, A, G) for f in fields)
    items = iu.sequence(unit, seed=11, zero=True, first=first)
    big = max(it.n for it in items)
    assert big * unit >= iu.BIG_BYTES and iu.neighbours(it.kind for it in items) >= {("B", "s"), ("s", "B"), ("B", "B")}
    gts = genotypes(items)
    tables = [] if disc else None
    sync = one_at_a_time(args, items, gts, fields, tables=tables)
    for got in sync:                                         # no site is skipped: every site's arrays are results
        assert (got["site_status"] >= 0).all()
    if with_oracle:
        against_the_oracle(oracle, args, items, gts, sync, fields)
    sim = Simulator(args, N, device=0, max_sites_per_tile=big)
    if disc:
        sim.discordance(1)
    mem = Pinned(lib, pageable)
    sets = [DestSet(mem, fields, big, A, G) for _ in range(2)]
    tickets = [C.c_int32(), C.c_int32()]
    found = []
    sides = []                                               # armed for the big tiles only
    bigs = [k for k, it in enumerate(items) if it.kind == "B"]
    if fetch:
        sim.fetch_gl(*fetch)
        sides.append(Side("fetched", mem, _abi.FetchGlTile, lib.vgl_ctx_fetchgl_next, int(lib.vgl_ctx_fetchgl_bound(sim.ctx, big)), big,
                          {k: fetched_of(args, sync[k], *fetch) for k in bigs}))
    if pile:
        read_cap = sim.info()["read_cap"]
        sides.append(Side("pileup", mem, _abi.PileupTile, lib.vgl_ctx_pileup_next, int(lib.vgl_ctx_pileup_bound(sim.ctx, big)), big,
                          {k: piled_of(args, items[k], gts[k], read_cap) for k in bigs}))

    def submit(k):
        S = sets[k & 1]
        if items[k].kind == "B":
            for sd in sides:
                sd.req[k & 1].text_needed = -7
                sim._check(sd.arm(sim.ctx, C.byref(sd.req[k & 1])))
        sim._check(lib.vgl_simulate_tile_async(sim.ctx, items[k].first, items[k].n, gts[k].ctypes.data, C.byref(S.struct), C.byref(tickets[k & 1])))

    def after(k, rc):
        d = sets[k & 1].dests(items[k].n)
        wants = dict(sync[k])
        mine = sides if items[k].kind == "B" else []
        for sd in mine:
            d[sd.name + " text"], d[sd.name + " offsets"] = (sd.text[k & 1], len(sd.want[k][0])), (sd.off[k & 1], 8 * (items[k].n + 1))
            wants[sd.name + " text"], wants[sd.name + " offsets"] = sd.want[k]
        snap = iu.tails(d)
        assert rc == _abi.VGL_OK, (k, lib.vgl_last_error())
        found.extend(f"item {k} ({items[k].kind}): {x}" for x in iu.late(snap, d, settled(args, wants, d)))
        for f, (a, used) in d.items():
            assert iu.untouched_behind(a, used), (k, f)
        sets[k & 1].poison(items[k].n)                       # item k + 2 is given these buffers next
        for sd in mine:
            assert sd.req[k & 1].text_needed == len(sd.want[k][0]), (k, sd.name)
            iu.poison(sd.text[k & 1][:len(sd.want[k][0])], sd.off[k & 1][:items[k].n + 1])

    waits = record_loop(items, submit, lambda k: lib.vgl_tile_wait(sim.ctx, tickets[k & 1]), after)
    show(name, items, waits)
    table = sim.discordance_table() if disc else None
    sim.close()
    mem.close()
    assert not found, found
    if disc:                                                 # the tally of the sequence: the model on (a)'s planes, and the tiles' own tables summed
        import disc_model as dm
        want = np.zeros(dm.table_len(N), dtype=np.int64)
        for got, gt in zip(sync, gts):
            if gt.shape[0]:
                dm.tally(got["site_status"], got["n_alleles"], got["alleles2acgt"], got["fmt_dp"], got["pl"], gt, table=want)
        assert want.any() and np.array_equal(table, want) and np.array_equal(table, np.sum(tables, axis=0))


def test_discordance_tally_with_tiles_in_flight(oracle):
    """vgl_ctx_discordance(ctx, 1): the table read after the sequence equals disc_model on the planes of (a), and the sum of the
    tables of the tiles run one by one"""
    run_plain(oracle, "plain tiles with the discordance tally", tile_args(seed=49), PLANE_FIELDS, with_oracle=False, disc=True)


def test_fetched_gl_of_the_big_tiles(oracle):
    """vgl_ctx_fetchgl_next armed for the big tiles only, a small tile behind each: text and offsets equal the stateless formatter on
    the planes of (a); the tiles' own outputs are what they are without the request"""
    run_plain(oracle, "plain tiles, GL fetched for the big ones", tile_args(seed=50), PLANE_FIELDS, with_oracle=False, fetch=(0, 1))


def test_pileup_of_the_big_tiles(oracle):
    """vgl_ctx_pileup_next armed for the big tiles only, a small tile behind each (finish_pileup and its copy on the text stream):
    text, offsets and text_needed equal the stateless pileup formatter on the read dump of the same tile run alone"""
    run_plain(oracle, "plain tiles, pileup of the big ones", tile_args(seed=52), PLANE_FIELDS, with_oracle=False, pile=True)


def test_plain_tiles_planes(oracle):
    run_plain(oracle, "plain tiles, planes", tile_args(), PLANE_FIELDS)


def test_plain_tiles_planes_pageable_destinations(oracle):
    run_plain(oracle, "plain tiles, planes, pageable destinations", tile_args(seed=43), PLANE_FIELDS, pageable=True)


def test_plain_tiles_sample_major_with_pl_u8(oracle):
    run_plain(oracle, "plain tiles, sample-major + pl_u8", tile_args(seed=44, out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR), PLANE_FIELDS + ["pl_u8"])


def test_plain_tiles_serial_mode(oracle):
    """serial RNG mode: the stream carries over from tile to tile, so order on the compute stream is part of the result -- held
    against the same order one at a time on a fresh context, and against nothing else"""
    run_plain(oracle, "plain tiles, serial mode", tile_args(seed=45, rng_mode=_abi.VGL_RNG_SERIAL, error_qs=0, beta_variance=-1.0), PLANE_FIELDS,
              with_oracle=False, first=0)


def test_a_device_error_in_a_small_tile_between_two_big_ones(oracle):
    """quality scores outside --qs-bins (as in test_gpu_parity's async case).  The big tiles hold missing genotypes only -- no read is
    drawn, so no score can miss a bin -- and the small tile between them real ones: the miss is reported by that tile's wait and by
    no other.  The two big tiles share a destination set and hold the same bytes (every site of an all-missing tile looks alike), so
    the set is poisoned again after the first and both are read tail-first against the same tile run alone, which is held against
    the oracle on 8 sites"""
    lib = _abi.load_library()
    args = tile_args(seed=46, qs_bins=[(0, 5, 3)])
    A, G = args.max_alleles, args.max_genotypes
    unit = sum(field_site_bytes(f, A, G) for f in PLANE_FIELDS)
    items = [it for it in iu.sequence(unit, seed=12, zero=False, first=500) if it.index in (0, 1, 3)]          # B s B
    assert [it.kind for it in items] == ["B", "s", "B"] and items[0].n * unit >= iu.BIG_BYTES
    gts = [np.full((it.n, N), 0xFF, np.uint8) if it.kind == "B" else np.ascontiguousarray(synth.binary_sites(it.first, 1, N)) for it in items]
    orc = oracle.Oracle(args, N)
    with pytest.raises(oracle.OracleError) as e:
        orc.simulate(items[1].first, gts[1], fields=PLANE_FIELDS)
    assert e.value.code == _abi.VGL_E_QSBIN
    big = items[0].n
    alone = {k: one_at_a_time(args, [items[k]], [gts[k]], PLANE_FIELDS)[0] for k in (0, 2)}
    against_the_oracle(oracle, args, [items[0], items[2]], [gts[0], gts[2]], [alone[0], alone[2]], PLANE_FIELDS)
    sim = Simulator(args, N, device=0, max_sites_per_tile=big)
    mem = Pinned(lib)
    sets = [DestSet(mem, PLANE_FIELDS, big, A, G) for _ in range(2)]
    tickets = [C.c_int32(), C.c_int32()]
    rcs, found = {}, []

    def submit(k):
        sim._check(lib.vgl_simulate_tile_async(sim.ctx, items[k].first, items[k].n, gts[k].ctypes.data, C.byref(sets[k & 1].struct), C.byref(tickets[k & 1])))

    def after(k, rc):
        d = sets[k & 1].dests(items[k].n)
        snap = iu.tails(d)
        rcs[k] = rc
        if items[k].kind == "B":
            found.extend(f"item {k}: {x}" for x in iu.late(snap, d, alone[k]))
            for f, (a, used) in d.items():
                assert iu.untouched_behind(a, used), (k, f)
        sets[k & 1].poison(items[k].n)

    waits = record_loop(items, submit, lambda k: lib.vgl_tile_wait(sim.ctx, tickets[k & 1]), after)
    show("device error in the small tile", items, waits)
    assert rcs == {0: _abi.VGL_OK, 1: _abi.VGL_E_QSBIN, 2: _abi.VGL_OK}
    assert not found, found
    sim.close()
    mem.close()
    orc.close()


# ---- 2. and 4. text tiles, and the deep rerun with a tile in flight ------------------------------------------------------------------------

def text_of(args, planes):
    """the stateless formatter (vcftext.format_columns) on host planes: (text bytes as uint8, offsets int64)"""
    n = planes["site_status"].shape[0]
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    dev = {f: torch.from_numpy(np.ascontiguousarray(a)).cuda() for f, a in planes.items()}
    text, off = vcftext.format_columns(vcftext.tile_fields(args, dev), dev["site_status"], dev["n_alleles"], N)
    return text.cpu().numpy(), off.cpu().numpy()


def text_sequence(args, seed, first, missing_small=False):
    """items whose big tiles format at least 64 MiB of text: the size of a site's text is taken from (a)'s own text of 64 sites, with
    five per cent to spare; the byte condition itself is asserted on every big tile's offsets.  missing_small: the small tiles hold missing
    genotypes (no read, so nothing to run again)"""
    probe_gt = np.ascontiguousarray(synth.binary_sites(first, 64, N))
    probe = one_at_a_time(args, [iu.Item(0, "s", 64, first, 0)], [probe_gt], PLANE_FIELDS)[0]
    per_site = len(text_of(args, probe)[0]) / 64
    items = iu.sequence(int(per_site * 0.95), seed=seed, zero=True, first=first)
    gts = genotypes(items)
    if missing_small:
        gts = [np.full_like(g, 0xFF) if it.kind == "s" else g for it, g in zip(items, gts)]
    return items, gts


def run_text(name, args, items, gts, sync, hooks=False):
    """the text sequence through vgl_simulate_tile_text_async, held against `sync` = [(planes, text, offsets)] of (a)"""
    lib = _abi.load_library(hooks=hooks)
    A, G = args.max_alleles, args.max_genotypes
    big = max(it.n for it in items)
    sim = Simulator(args, N, device=0, max_sites_per_tile=big, hooks=hooks)
    if hooks:
        assert sim.info()["read_cap"] == 8
    cap = int(lib.vgl_ctx_text_bound(sim.ctx, big))
    mem = Pinned(lib)
    sets = [DestSet(mem, SITE_FIELDS, big, A, G) for _ in range(2)]
    texts = [mem.array((cap,), np.uint8) for _ in range(2)]
    offs = [mem.array((big + 1,), np.int64) for _ in range(2)]
    iu.poison(*texts, *offs)
    tickets = [C.c_int32(), C.c_int32()]
    found = []

    def submit(k):
        s = k & 1
        sim._check(lib.vgl_simulate_tile_text_async(sim.ctx, items[k].first, items[k].n, gts[k].ctypes.data, C.byref(sets[s].struct),
                                                     texts[s].ctypes.data, cap, offs[s].ctypes.data, C.byref(tickets[s])))

    def after(k, rc):
        s, n = k & 1, items[k].n
        planes, text, off = sync[k]
        d = sets[s].dests(n)
        d["text"] = (texts[s], len(text))
        d["offsets"] = (offs[s], 8 * (n + 1))
        snap = iu.tails(d)
        assert rc == _abi.VGL_OK, (k, lib.vgl_last_error())
        wants = {f: planes[f] for f in SITE_FIELDS}
        wants["text"], wants["offsets"] = text, off
        found.extend(f"item {k} ({items[k].kind}): {x}" for x in iu.late(snap, d, wants))
        assert iu.untouched_behind(texts[s], len(text)), (k, "bytes behind offsets[n] were written")
        assert iu.untouched_behind(offs[s], 8 * (n + 1)), k
        sets[s].poison(n)                                    # item k + 2 is given these buffers next
        iu.poison(texts[s][:len(text)], offs[s][:n + 1])

    waits = record_loop(items, submit, lambda k: lib.vgl_tile_wait(sim.ctx, tickets[k & 1]), after)
    show(name, items, waits)
    info = sim.info()
    sim.close()
    mem.close()
    assert not found, found
    return info


def text_reference(args, items, gts):
    sync = []
    for planes in one_at_a_time(args, items, gts, PLANE_FIELDS):
        text, off = text_of(args, planes)
        sync.append((planes, text, off))
    for it, (_, text, off) in zip(items, sync):
        assert int(off[-1]) == len(text)
        if it.kind == "B":
            assert len(text) >= iu.BIG_BYTES, (it, len(text))              # the byte condition
    return sync


@pytest.fixture(scope="module")
def text_case():
    """one text sequence and its (a), shared and left unchanged: (args, items, gts, [(planes, text, offsets)])"""
    args = tile_args(seed=47, out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR)
    items, gts = text_sequence(args, seed=13, first=3000)
    return args, items, gts, text_reference(args, items, gts)


def test_text_tiles(oracle, text_case):
    """GL + PL + DP as text into a host destination: text and offsets of every tile equal vcftext.format_columns on the planes of (a),
    the bytes behind offsets[n] are still poison, the returned per-site arrays are equal too"""
    args, items, gts, sync = text_case
    against_the_oracle(oracle, args, items, gts, [p for p, _, _ in sync], PLANE_FIELDS)
    run_text("text tiles", args, items, gts, sync)


GVCF_FIELDS = ["site_status", "n_alleles", "n_alleles_obs", "alleles2acgt", "fmt_dp"]
GVCF_DPS = [1, 3, 5]


def hom_ref_sites(n, seed):
    """every sample homozygous for the site's own reference allele: sites stay invariant unless an error is drawn, so blocks form"""
    if n == 0:
        return np.zeros((0, N), np.uint8)
    ref = synth.acgt_sites(n, 1, seed=seed, missing=0.0) & 0x0F
    return np.ascontiguousarray((ref | (ref << 4)).repeat(N, axis=1).astype(np.uint8))


def blocked_of(args, planes, contig, pos0):
    """the synchronous blocker (vgl_gvcf_blocks_device) and the stateless formatter on host planes, as tests/test_gpu_gvcf.py holds its
    record loop: ({destination: wanted bytes}, (n_items, n_blocks, error_site), the first / last block's DP and PL or None)"""
    from vcfgl_amd import gvcf
    n = planes["site_status"].shape[0]
    dev = {f: torch.from_numpy(np.ascontiguousarray(a)).cuda() for f, a in planes.items()}
    pl = dev["pl"].reshape(n, -1)
    r = gvcf.blocks_device_raw(GVCF_DPS, dev["site_status"], dev["n_alleles_obs"], dev["n_alleles"], torch.from_numpy(contig).cuda(),
                               torch.from_numpy(pos0).cuda(), dev["fmt_dp"], pl)
    rtext, roff = vcftext.format_columns(vcftext.tile_fields(args, dev), r["record_status"][:n], dev["n_alleles"], N)
    bfields = [("PL", r["block_pl"][:n], vcftext.PER_G), ("DP", r["block_dp"][:n], vcftext.ONE)]
    btext, boff = vcftext.format_columns(bfields, r["block_status"][:n], r["block_n_alleles"][:n], N)
    roff, boff = roff.cpu().numpy(), boff.cpu().numpy()
    want = {"text": np.concatenate([rtext.cpu().numpy(), btext.cpu().numpy()]), "record offsets": roff, "block offsets": boff + int(roff[-1]),
            "items": np.array(r["items"].tolist(), dtype=np.int32).reshape(-1)}
    for f in GVCF_FIELDS:
        want[f] = planes[f]
    nb, edges = r["n_blocks"], None
    if nb:
        edges = (r["block_dp"][0].cpu().numpy(), r["block_dp"][nb - 1].cpu().numpy(), r["block_pl"][0].cpu().numpy()[:3 * N],
                 r["block_pl"][nb - 1].cpu().numpy()[:3 * N])
    return want, (r["n_items"], nb, r["error_site"]), edges


def test_gvcf_tiles():
    """vgl_simulate_tile_gvcf_async on one sequence (a -doGVCF 1 context: sample-major, DP and PL): the items, the counts, the text of
    records and blocks, both offset arrays, text_needed, the first and last block's aggregates and the per-site arrays equal the
    synchronous blocker and formatter on the planes of (a).  Big: the DP, GL and PL planes a tile writes on the device are at least
    64 MiB.  copy_gvcf_small copies n_sites items whatever n_items is, so of `items` the first n_items are held"""
    lib = _abi.load_library()
    # depth 14: no sample of 500 stays without a read, so a site's smallest DP reaches a block threshold; 7000 reads a site at this
    # error rate leave two sites in three invariant (the oracle on 300 such sites: 142 blocks and 96 records)
    args = VcfglArgs(seed=51, depth=14, error_rate=5e-5, do_unobserved=2, add_pl=1, do_gvcf=1)
    args.rng_mode, args.beta_sampler, args.out_layout = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48, _abi.VGL_LAYOUT_SAMPLE_MAJOR
    A, G = args.max_alleles, args.max_genotypes
    unit = sum(field_site_bytes(f, A, G) for f in ("fmt_dp", "gl", "pl"))
    items = iu.sequence(unit, seed=20, zero=True, first=100)
    big = max(it.n for it in items)
    assert big * unit >= iu.BIG_BYTES
    gts = [hom_ref_sites(it.n, it.seed) for it in items]
    contigs = [np.zeros(max(it.n, 1), np.int32) for it in items]
    pos0s = [it.first + np.arange(max(it.n, 1), dtype=np.int64) for it in items]
    planes = one_at_a_time(args, items, gts, GVCF_FIELDS + ["gl", "pl"])
    sync = [blocked_of(args, pl, c[:it.n], p0[:it.n]) if it.n else None for it, pl, c, p0 in zip(items, planes, contigs, pos0s)]
    print("\ngVCF tiles: (n_items, n_blocks, error_site) of (a):", [w[1] if w else None for w in sync])
    assert all(w[1][1] > 2 for it, w in zip(items, sync) if it.kind == "B"), "a big tile built no blocks"
    dps_a = (C.c_int32 * len(GVCF_DPS))(*GVCF_DPS)
    sim = Simulator(args, N, device=0, max_sites_per_tile=big)
    cap = int(lib.vgl_ctx_gvcf_text_bound(sim.ctx, big))
    mem = Pinned(lib)
    sets = [DestSet(mem, GVCF_FIELDS, big, A, G) for _ in range(2)]
    bufs = [dict(text=mem.array((cap,), np.uint8), roff=mem.array((big + 1,), np.int64), boff=mem.array((big + 1,), np.int64),
                 items=mem.array((8 * big,), np.int32), fdp=mem.array((N,), np.int32), ldp=mem.array((N,), np.int32),
                 fpl=mem.array((N * G,), np.int32), lpl=mem.array((N * G,), np.int32)) for _ in range(2)]
    for b in bufs:
        iu.poison(*b.values())
    reqs, tickets, found = [None, None], [C.c_int32(), C.c_int32()], []

    def submit(k):
        s, it, b = k & 1, items[k], bufs[k & 1]
        reqs[s] = _abi.GvcfTile(b["items"].ctypes.data, b["text"].ctypes.data, cap, b["roff"].ctypes.data, b["boff"].ctypes.data, b["fdp"].ctypes.data,
                                b["fpl"].ctypes.data, b["ldp"].ctypes.data, b["lpl"].ctypes.data, 0, 0, 0, 0, 0)
        sim._check(lib.vgl_simulate_tile_gvcf_async(sim.ctx, it.first, it.n, gts[k].ctypes.data, contigs[k].ctypes.data, pos0s[k].ctypes.data, dps_a,
                                                     len(GVCF_DPS), C.byref(sets[s].struct), C.byref(reqs[s]), C.byref(tickets[s])))

    def after(k, rc):
        s, n, b, g = k & 1, items[k].n, bufs[k & 1], reqs[k & 1]
        if sync[k] is None:
            assert rc == _abi.VGL_OK and b["roff"][0] == 0 and b["boff"][0] == 0, (k, lib.vgl_last_error())
            assert (g.n_items, g.n_blocks, g.error_site, g.text_needed) == (0, 0, -1, 0)
            iu.poison(b["roff"][:1], b["boff"][:1])
            return
        want, counts, edges = sync[k]
        d = sets[s].dests(n)
        d["text"] = (b["text"], len(want["text"]))
        d["record offsets"], d["block offsets"] = (b["roff"], 8 * (n + 1)), (b["boff"], 8 * (n + 1))
        d["items"] = (b["items"], 4 * len(want["items"]))
        snap = iu.tails(d)
        assert rc == _abi.VGL_OK, (k, lib.vgl_last_error())
        found.extend(f"item {k} ({items[k].kind}): {x}" for x in iu.late(snap, d, want))
        assert (g.n_items, g.n_blocks, g.error_site) == counts and g.text_needed == len(want["text"]), k
        for f in ("text", "record offsets", "block offsets"):
            assert iu.untouched_behind(*d[f]), (k, f)
        if edges:
            assert np.array_equal(b["fdp"], edges[0]) and np.array_equal(b["ldp"], edges[1]), k
            assert np.array_equal(b["fpl"][:3 * N], edges[2]) and np.array_equal(b["lpl"][:3 * N], edges[3]), k
        sets[s].poison(n)                                    # item k + 2 is given these buffers next
        iu.poison(b["text"][:len(want["text"])], b["roff"][:n + 1], b["boff"][:n + 1], b["items"][:8 * n], b["fdp"], b["ldp"], b["fpl"], b["lpl"])

    waits = record_loop(items, submit, lambda k: lib.vgl_tile_wait(sim.ctx, tickets[k & 1]), after)
    show("gVCF tiles", items, waits)
    sim.close()
    mem.close()
    assert not found, found


# ---- 5. device-resident text into the stream handle, two threads ---------------------------------------------------------------------------

def site_heads(rng, n):
    """random heads of 0 .. 200 bytes per site: (bytes, offsets)"""
    hl = rng.integers(0, 201, n)
    return rng.integers(0, 256, int(hl.sum()), dtype=np.uint8), np.concatenate([[0], np.cumsum(hl)]).astype(np.int64)


@pytest.mark.parametrize("n_buffers", [2, 3])
def test_device_text_into_the_stream_handle_from_two_threads(text_case, n_buffers):
    """vgl_ctx_text_device + vgl_stream_host_*: this thread drives the tiles into body buffer k = tile mod n_buffers (two tiles in
    flight on the context), a second thread takes (tile, k, offsets, heads) from a queue, submits to the stream handle and waits in
    submit order (n_buffers - 1 tickets in flight).  This thread learns through the reply queue that buffer k's ticket has been waited
    for before it writes k again.  The members of all tiles, joined and inflated by zlib, equal stream_model.assemble of the heads and
    the text of (a); every tile's members are cut where bgzf_model cuts them, its first and last equal bgzf_model's bit for bit"""
    from vcfgl_amd import stream
    args, items, gts, sync = text_case
    lib = _abi.load_library()
    A, G = args.max_alleles, args.max_genotypes
    big = max(it.n for it in items)
    sim = Simulator(args, N, device=0, max_sites_per_tile=big)
    cap = int(lib.vgl_ctx_text_bound(sim.ctx, big))
    sim._check(lib.vgl_ctx_text_device(sim.ctx, 1))
    heads = [site_heads(np.random.default_rng(it.seed), it.n) for it in items]
    hs = stream.HostStream(0, n_buffers, big, 200 * big + 1, cap)
    mem = Pinned(lib)
    sets = [DestSet(mem, SITE_FIELDS, big, A, G) for _ in range(2)]
    offs = [mem.array((big + 1,), np.int64) for _ in range(2)]
    iu.poison(*offs)
    tickets = [C.c_int32(), C.c_int32()]
    jobs, replies, results, found, errors = queue.Queue(), queue.Queue(), {}, [], []

    def writer():
        """the second thread: submit, then wait in submit order with at most n_buffers - 1 tickets in flight"""
        pending = []

        def finish():
            k, ticket = pending.pop(0)
            p, m, raw = C.c_void_p(), C.c_int64(), C.c_int64()
            rc = lib.vgl_stream_host_wait(hs.h, ticket, C.byref(p), C.byref(m), C.byref(raw))
            v = view(p.value, m.value if rc == _abi.VGL_OK else 0)
            tail = v[max(0, v.size - iu.TAIL):].copy()       # first the tail, then the whole
            results[k] = (rc, tail, v.copy(), raw.value)
            replies.put(k)

        try:
            while True:
                job = jobs.get()
                if job is None:
                    break
                k, b, off, (hb, ho) = job
                hb, ho = hb.copy(), ho.copy()
                t = C.c_int32(-1)
                rc = lib.vgl_stream_host_submit(hs.h, b, items[k].n, hb.ctypes.data, ho.ctypes.data, off.ctypes.data, C.byref(t))
                assert rc == _abi.VGL_OK, lib.vgl_last_error()
                hb[:] = 0xEE; ho[:] = -1; off[:] = -1        # heads and offsets are free again on return from submit
                pending.append((k, t.value))
                while len(pending) > n_buffers - 2:
                    finish()
            while pending:
                finish()
        except BaseException as e:                           # (reported by the test's thread)
            errors.append(e)
            replies.put(None)

    th = threading.Thread(target=writer)
    th.start()
    waited = set()

    def buffer_is_free(k):
        """tile k - n_buffers has been waited for by the writer: learnt through its reply"""
        while k - n_buffers >= 0 and k - n_buffers not in waited:
            r = replies.get()
            assert r is not None, errors
            waited.add(r)

    def submit(k):
        s = k & 1
        buffer_is_free(k)
        sim._check(lib.vgl_simulate_tile_text_async(sim.ctx, items[k].first, items[k].n, gts[k].ctypes.data, C.byref(sets[s].struct),
                                                     hs.body(k % n_buffers), cap, offs[s].ctypes.data, C.byref(tickets[s])))

    def after(k, rc):
        s, n = k & 1, items[k].n
        planes, text, off = sync[k]
        d = sets[s].dests(n)
        d["offsets"] = (offs[s], 8 * (n + 1))
        snap = iu.tails(d)
        assert rc == _abi.VGL_OK, (k, lib.vgl_last_error())
        wants = {f: planes[f] for f in SITE_FIELDS}
        wants["offsets"] = off
        found.extend(f"item {k} ({items[k].kind}): {x}" for x in iu.late(snap, d, wants))
        jobs.put((k, k % n_buffers, offs[s][:n + 1].copy(), heads[k]))
        sets[s].poison(n)                                    # item k + 2 is given these buffers next
        iu.poison(offs[s][:n + 1])

    try:
        waits = record_loop(items, submit, lambda k: lib.vgl_tile_wait(sim.ctx, tickets[k & 1]), after)
    finally:
        jobs.put(None)
        th.join()
    show(f"device text into the stream handle, {n_buffers} buffers", items, waits)
    assert not errors, errors
    assert not found, found
    for k, it in enumerate(items):                           # (every member of every tile inflated by zlib: so is their concatenation)
        rc, tail, members, raw = results[k]
        assert rc == _abi.VGL_OK, k
        want, _ = sm.assemble(heads[k][0], heads[k][1], sync[k][1], sync[k][2])
        assert raw == len(want), k
        assert np.array_equal(tail, members[max(0, members.size - iu.TAIL):]), (k, "the members' tail was not there when the wait returned")
        if it.n:
            sampled_members_equal_the_model(members, want, count=2)
        else:
            assert members.size == 0
    hs.close()
    sim.close()
    mem.close()


def test_deep_rerun_with_a_tile_in_flight(monkeypatch):
    """VGL_DEBUG_READ_CAP=8 at depth 20 (hooks build, as test_deep_rerun_gives_the_same_text): every big tile of a text sequence is run
    again by vgl_tile_wait while the next tile is already enqueued; text, offsets and fmt_dp equal the run without the hook.  Every
    big tile holds a depth above 8, which the first run at a staging capacity of 8 cannot deliver: the equal bytes are the rerun's.
    (The context's count of reruns is not exported by vgl_ctx_info, so it is not read.)  The small tiles hold missing genotypes: no
    read is drawn, so they are not run again"""
    args = tile_args(seed=48, depth=20, out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR)
    items, gts = text_sequence(args, seed=14, first=7000, missing_small=True)
    sync = text_reference(args, items, gts)                          # (without the hook: the shipped build)
    assert all(int(p["fmt_dp"].max()) > 8 for it, (p, _, _) in zip(items, sync) if it.kind == "B")
    assert all(int(p["fmt_dp"].max()) == 0 for it, (p, _, _) in zip(items, sync) if it.kind == "s")
    monkeypatch.setenv("VGL_DEBUG_READ_CAP", "8")
    run_text("deep rerun, text tiles", args, items, gts, sync, hooks=True)


# ---- 6. the five host-batch families ----------------------------------------------------------------------------------------------------

def ok(lib, rc):
    assert rc == _abi.VGL_OK, lib.vgl_last_error()


def scribble(*arrays):
    """garbage over inputs that are free again on return from submit: every byte of a small array, one byte in every 4 KiB of a large
    one (filling 64 MiB takes longer than the batch: it would stand between the submit and the wait that is to be observed)"""
    for a in arrays:
        b = iu.as_bytes(a)
        if b.size <= 1 << 16:
            b[:] = 0xEE
        else:
            b[::4096] ^= 0xEE


def view(ptr, nbytes):
    """the handle's own result memory as a uint8 array"""
    if not nbytes:
        return np.zeros(0, np.uint8)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(int(nbytes),))


@pytest.fixture(scope="module")
def pool():
    """64 MiB and a little of compressible text-like bytes, drawn once: an item's content is a window of it at its own offset"""
    rng = np.random.default_rng(61)
    alphabet = np.frombuffer(b"0123456789.|/:\t\n-,ACGT", np.uint8)
    return alphabet[rng.integers(0, len(alphabet), iu.BIG_BYTES + (1 << 20), dtype=np.uint8)]


def sampled_members_equal_the_model(members, data, count=4):
    """zlib inflates every member to its input and the members end where bgzf_model's do (every MEMBER input bytes); `count` members
    (first, last, between) equal bgzf_model's bit for bit"""
    parts = bgzf_model.split_members(bytes(members))
    assert [int.from_bytes(g[-4:], "little") for g in parts] == [M] * (len(data) // M) + ([len(data) % M] if len(data) % M else [])
    at = 0
    for g in parts:
        piece = zlib.decompress(g[18:-8], -15)
        assert piece == bytes(data[at:at + len(piece)]) and int.from_bytes(g[-8:-4], "little") == zlib.crc32(piece)
        at += len(piece)
    assert at == len(data)
    for j in iu.sample_sites(len(parts), count):
        assert parts[j] == bgzf_model.compress(bytes(data[j * M:(j + 1) * M])), j


class Family:
    """one family's sequence: submit(h, k) -> ticket, result(h, ticket, k) -> {name: (view of the handle's memory, bytes)} straight
    after the wait, anchor(k, got) holds (a) against zlib / the CPU model"""
    zero = True

    def run(self, name):
        lib = self.lib
        h = self.create()
        sync = []
        for k in range(len(self.items)):                    # (a): submit then wait with nothing else in flight
            d = self.result(h, self.submit(h, k), k)
            sync.append({f: a[:n].copy() for f, (a, n) in d.items()})
            self.anchor(k, sync[-1])
        ok(lib, self.destroy(h))
        h = self.create()
        tickets, found, live = {}, [], {}

        def submit(k):
            tickets[k] = self.submit(h, k)

        def after(k, d):
            snap = iu.tails(d)
            wants = self.wanted(k, sync[k], d)
            found.extend(f"item {k} ({self.items[k].kind}): {x}" for x in iu.late(snap, d, wants))
            for a, n in d.values():                          # the slot's result memory is poisoned for the batch after the next
                a[:n] = iu.POISON

        def wait(k):
            live[k] = self.result(h, tickets[k], k)
            return live[k]

        waits = record_loop(self.items, submit, wait, after)
        show(name, self.items, waits)
        # a third submit without a wait is still refused, and the handle still works
        t0, t1 = self.submit(h, 1), self.submit(h, 2)
        assert self.submit_rc(h, 1, prepare=False)[0] == _abi.VGL_E_ARG and b"in flight" in lib.vgl_last_error()
        for t, k in ((t0, 1), (t1, 2)):
            d = self.result(h, t, k)
            assert iu.late(iu.tails(d), d, self.wanted(k, sync[k], d)) == []
        ok(lib, self.destroy(h))
        assert not found, found

    def wanted(self, k, sync_k, d):
        return sync_k

    def submit(self, h, k):
        rc, t = self.submit_rc(h, k)
        ok(self.lib, rc)
        return t


class BgzfFamily(Family):
    def __init__(self, pool):
        self.lib, self.pool = _abi.load_library(), pool
        self.items = iu.sequence(1, seed=15, zero=True)
        self.mem = Pinned(self.lib)
        self.src = [self.mem.array((iu.BIG_BYTES,), np.uint8) for _ in range(2)]         # page-locked sources, one per slot

    def data(self, k):
        it = self.items[k]
        return self.pool[977 * it.index:977 * it.index + it.n]

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_bgzf_host_create(0, iu.BIG_BYTES, C.byref(h)))
        self.turn = 0
        return h

    def submit_rc(self, h, k, prepare=True):
        s, n = self.src[self.turn & 1], self.items[k].n        # src stays unchanged until its ticket is waited for: the slot's own buffer
        if prepare:                                          # (a submit that will be refused must not write a source in flight)
            s[:n] = self.data(k)
        t = C.c_int32(-1)
        rc = self.lib.vgl_bgzf_host_submit(h, s.ctypes.data, n, C.byref(t))
        if rc == _abi.VGL_OK:
            self.turn += 1
        return rc, t.value

    def result(self, h, ticket, k):
        out, n = C.c_void_p(), C.c_int64()
        ok(self.lib, self.lib.vgl_bgzf_host_wait(h, ticket, C.byref(out), C.byref(n)))
        return {"members": (view(out.value, n.value), n.value)}

    def anchor(self, k, got):
        sampled_members_equal_the_model(got["members"], self.data(k))

    def destroy(self, h):
        return self.lib.vgl_bgzf_host_destroy(h)


def test_bgzf_host_batches(pool):
    f = BgzfFamily(pool)
    assert max(it.n for it in f.items) >= iu.BIG_BYTES
    try:
        f.run("bgzf host batches")
    finally:
        f.mem.close()


class InflateFamily(Family):
    """members of MEMBER input bytes at zlib level 1, compressed once; a big batch is a window of them at its own offset"""

    def __init__(self, pool):
        self.lib = _abi.load_library()
        self.items = iu.sequence(M, seed=16, zero=True)
        big = max(it.n for it in self.items)
        assert big * M >= iu.BIG_BYTES
        n_members = big + len(self.items)
        assert n_members * M <= len(pool)
        self.pieces = [bytes(pool[j * M:(j + 1) * M]) for j in range(n_members)]
        self.members = [ic.wrap(ic.deflate(p, level=1), p) for p in self.pieces]
        self.max_members = big

    def window(self, k):
        it = self.items[k]
        return range(it.index, it.index + it.n)

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_inflate_host_create(0, self.max_members, C.byref(h)))
        return h

    def submit_rc(self, h, k, prepare=True):
        w = self.window(k)
        raw = b"".join(self.members[j] for j in w)
        csize = np.array([len(self.members[j]) for j in w], np.int32)
        begin = np.concatenate([[0], np.cumsum(csize[:-1])]).astype(np.int64) if len(w) else np.zeros(0, np.int64)
        isize = np.full(len(w), M, np.int32)
        src = np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(1, np.uint8)
        t = C.c_int32(-1)
        rc = self.lib.vgl_inflate_host_submit(h, src.ctypes.data, len(raw), len(w), begin.ctypes.data, csize.ctypes.data, isize.ctypes.data, C.byref(t))
        scribble(src, begin, csize, isize)                   # submit has copied the batch into its staging: the caller's arrays are free
        return rc, t.value

    def result(self, h, ticket, k):
        out, n, st = C.c_void_p(), C.c_int64(), C.c_void_p()
        ok(self.lib, self.lib.vgl_inflate_host_wait(h, ticket, C.byref(out), C.byref(n), C.byref(st)))
        m = len(self.window(k))
        return {"bytes": (view(out.value, n.value), n.value), "status": (view(st.value, 4 * m), 4 * m)}

    def anchor(self, k, got):
        w = self.window(k)
        assert bytes(got["bytes"]) == b"".join(zlib.decompress(ic.deflate_of(self.members[j]), -15) for j in w)
        assert not got["status"].any()

    def destroy(self, h):
        return self.lib.vgl_inflate_host_destroy(h)


def test_inflate_host_batches(pool):
    InflateFamily(pool).run("inflate host batches")


class Repeated:
    """a batch built by repeating the lines (records) of small cases: parts = [(case, repetitions)], shift = the positions in
    case.arrays() of the arrays that hold offsets into the text (bytes)"""

    def __init__(self, parts, shift):
        datas, cols, rows, sums, status, at = [], None, [], [], [], 0
        for case, reps in parts:
            data, *arrs = case.arrays()
            e = case.expected()
            datas.append(bytes(data) * reps)
            step = len(data) * np.arange(reps, dtype=np.int64)[:, None]
            out = []
            for j, a in enumerate(arrs, start=1):
                a = np.asarray(a)
                t = np.tile(a[None], (reps,) + (1,) * a.ndim)
                if j in shift:
                    t = t + step + at
                out.append(t.reshape((-1,) + a.shape[1:]))
            cols = out if cols is None else [np.concatenate([c, o]) for c, o in zip(cols, out)]
            rows.append(np.tile(e[0], (reps, 1))); sums.append(np.tile(e[1], reps)); status.append(np.tile(e[2], reps))
            at += len(data) * reps
        self.data = np.frombuffer(b"".join(datas), np.uint8) if at else np.zeros(1, np.uint8)
        self.nbytes, self.cols = at, [np.ascontiguousarray(c) for c in cols]
        self.n = len(self.cols[0])
        self.expected = (np.concatenate(rows), np.concatenate(sums), np.concatenate(status))


class RowsFamily(Family):
    """vcfin / bcfin: rows [n][NS], sums and statuses; one line of every batch is handed back by the device"""
    NS = 1000

    def batch(self, k):
        if k not in self.cache:
            it = self.items[k]
            rng = np.random.default_rng(it.seed)
            plain, back = self.plain_case(rng), self.handed_back_case()
            if it.kind == "B":
                reps = -(-iu.BIG_BYTES // self.case_bytes(plain))
                self.cache[k] = Repeated([(plain, reps // 2), (back, 1), (plain, reps - reps // 2)], self.shift)
                assert self.batch_bytes(self.cache[k]) >= iu.BIG_BYTES
            elif it.kind == "s":
                self.cache[k] = Repeated([(back if it.index == 2 else self.plain_case(rng, 1), 1)], self.shift)
            else:
                self.cache[k] = None
        return self.cache[k]

    def submit_rc(self, h, k, prepare=True):
        b = self.batch(k)
        t = C.c_int32(-1)
        if b is None:
            return self.entry_submit(h, None, 0, 0, None, None, None, None, None, C.byref(t)), t.value
        data, cols = b.data.copy(), [c.copy() for c in b.cols]
        rc = self.entry_submit(h, data.ctypes.data, b.nbytes, b.n, *[c.ctypes.data for c in cols], C.byref(t))
        scribble(data, *cols)                                # submit has copied the batch into its staging: the caller's arrays are free
        return rc, t.value

    def result(self, h, ticket, k):
        g, s, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ok(self.lib, self.entry_wait(h, ticket, C.byref(g), C.byref(s), C.byref(st)))
        n = self.batch(k).n if self.batch(k) is not None else 0
        return {"rows": (view(g.value, n * self.NS), n * self.NS), "sums": (view(s.value, 4 * n), 4 * n), "status": (view(st.value, 4 * n), 4 * n)}

    def anchor(self, k, got):
        b = self.batch(k)
        if b is None:
            return
        rows, sums, status = b.expected
        good = status == 0
        assert int((~good).sum()) == (0 if self.items[k].kind == "s" and self.items[k].index != 2 else 1)
        assert np.array_equal(got["status"].view(np.int32), status)
        assert np.array_equal(got["rows"].reshape(b.n, self.NS)[good], rows[good]) and np.array_equal(got["sums"].view(np.int32)[good], sums[good])

    def wanted(self, k, sync_k, d):
        """the row and the sum of a line that is handed back are not results: taken as delivered"""
        b = self.batch(k)
        if b is None:
            return sync_k
        bad = np.flatnonzero(b.expected[2] != 0)
        want = {f: a.copy() for f, a in sync_k.items()}
        want["rows"].reshape(b.n, self.NS)[bad] = d["rows"][0][:b.n * self.NS].reshape(b.n, self.NS)[bad]
        want["sums"].view(np.int32)[bad] = d["sums"][0][:4 * b.n].view(np.int32)[bad]
        return want


class VcfinFamily(RowsFamily):
    shift = (1, 2)

    def __init__(self):
        self.lib, self.cache = _abi.load_library(), {}
        self.items = iu.sequence(1, seed=17, zero=True)      # (units: bytes of text; a batch is sized by its cases)
        self.entry_submit, self.entry_wait = self.lib.vgl_vcfin_host_submit, self.lib.vgl_vcfin_host_wait

    def plain_case(self, rng, lines=15):
        c = vc.Case(self.NS)
        for _ in range(lines):
            vc.random_line(c, rng)
        return c

    def handed_back_case(self):
        return vc.Case(self.NS).add([b"0|1"] * (self.NS - 1) + [b"0|x"], fallback=True)

    def case_bytes(self, c):
        return c.size

    def batch_bytes(self, b):
        return b.nbytes

    def create(self):
        h = C.c_void_p()
        big = [self.batch(k) for k, it in enumerate(self.items) if it.kind == "B"]
        ok(self.lib, self.lib.vgl_vcfin_host_create(0, self.NS, max(b.n for b in big), max(b.nbytes for b in big), C.byref(h)))
        return h

    def destroy(self, h):
        return self.lib.vgl_vcfin_host_destroy(h)


def test_vcfin_host_batches():
    VcfinFamily().run("vcfin host batches")


class BcfinFamily(RowsFamily):
    shift = (1,)

    def __init__(self):
        self.lib, self.cache = _abi.load_library(), {}
        self.items = iu.sequence(1, seed=18, zero=True)      # (units: GT bytes; a batch is sized by its cases)
        self.entry_submit, self.entry_wait = self.lib.vgl_bcfin_host_submit, self.lib.vgl_bcfin_host_wait

    def plain_case(self, rng, records=15):
        c = bc.Case(self.NS)
        for i in range(records):
            c.pad(int(rng.integers(0, 9)))
            bc.random_record(c, rng, gt_type=1 + i % 3, n=1 + i % 4)
        return c

    def handed_back_case(self):
        return bc.Case(self.NS).pad(3).add([[bc.gt_value(0), "M"]] * self.NS, fallback=True)

    def case_bytes(self, c):
        return sum(c.slice_bytes(i) for i in range(len(c.begin)))

    def batch_bytes(self, b):
        """the GT bytes of the batch: what crosses the link"""
        return int(sum(self.NS * int(n) * bm.WIDTH[int(t)] for t, n in zip(b.cols[1], b.cols[2])))

    def create(self):
        h = C.c_void_p()
        big = [self.batch(k) for k, it in enumerate(self.items) if it.kind == "B"]
        ok(self.lib, self.lib.vgl_bcfin_host_create(0, self.NS, max(b.n for b in big), max(self.batch_bytes(b) for b in big), C.byref(h)))
        return h

    def destroy(self, h):
        return self.lib.vgl_bcfin_host_destroy(h)


def test_bcfin_host_batches():
    BcfinFamily().run("bcfin host batches")


def to_raw(ptr, t):
    """copy the device tensor t to the raw device address ptr (a one-site stream: no head, t as the body)"""
    z = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, t.numel()], dtype=torch.int64, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib = _abi.load_library()
    ok(lib, lib.vgl_stream_assemble_device(0, 1, t.data_ptr(), z.data_ptr(), t.data_ptr(), off.data_ptr(), ptr, t.numel(), total.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(total.item()) == t.numel()


class StreamFamily(Family):
    """vgl_stream_host_* on its own: two body buffers filled from host bytes, heads of 0 .. 200 random bytes per site.  A big tile is
    sites of 65600 body bytes, a small one a site of 100"""
    BODY = 65600

    def __init__(self, pool):
        self.lib, self.pool = _abi.load_library(), pool
        self.items = iu.sequence(self.BODY, seed=19, zero=True)
        self.big = max(it.n for it in self.items)
        assert self.big * self.BODY >= iu.BIG_BYTES

    def tile(self, k):
        it = self.items[k]
        per = self.BODY if it.kind == "B" else 100
        hb, ho = site_heads(np.random.default_rng(it.seed), it.n)
        bodies = self.pool[613 * it.index:613 * it.index + it.n * per]
        return hb, ho, bodies, per * np.arange(it.n + 1, dtype=np.int64)

    def create(self):
        h = C.c_void_p()
        ok(self.lib, self.lib.vgl_stream_host_create(0, 2, self.big, 200 * self.big + 1, self.big * self.BODY, C.byref(h)))
        self.turn = 0
        return h

    def submit_rc(self, h, k, prepare=True):
        b = self.turn & 1
        hb, ho, bodies, bo = self.tile(k)
        if prepare and len(bodies):                          # (a submit that will be refused must not write a buffer in flight)
            to_raw(self.lib.vgl_stream_host_body(h, b), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        hb, ho = hb.copy(), ho.copy()
        t = C.c_int32(-1)
        rc = self.lib.vgl_stream_host_submit(h, b, self.items[k].n, hb.ctypes.data, ho.ctypes.data, bo.ctypes.data, C.byref(t))
        hb[:] = 0xEE; ho[:] = -1; bo[:] = -1                 # heads and offsets are free again on return from submit
        if rc == _abi.VGL_OK:
            self.turn += 1
        return rc, t.value

    def result(self, h, ticket, k):
        p, m, raw = C.c_void_p(), C.c_int64(), C.c_int64()
        ok(self.lib, self.lib.vgl_stream_host_wait(h, ticket, C.byref(p), C.byref(m), C.byref(raw)))
        self.raw = raw.value
        return {"members": (view(p.value, m.value), m.value)}

    def anchor(self, k, got):
        want, _ = sm.assemble(*self.tile(k))
        assert self.raw == len(want)
        if len(want):
            sampled_members_equal_the_model(got["members"], want)
        else:
            assert got["members"].size == 0

    def destroy(self, h):
        return self.lib.vgl_stream_host_destroy(h)


def test_stream_host_batches(pool):
    StreamFamily(pool).run("stream host batches")


# ---- 7. the program, at a size where tiles take milliseconds --------------------------------------------------------------------------------

CLI_S, CLI_N, CLI_TIMEOUT = 2048, 500, 120
CLI_REF = "--seed 42 --depth 2 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -addGL 1 -addPL 1 -addFormatDP 1 -printTruth 1".split()
CLI_STAGES = {"b": ["--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"], "z": ["--device-text", "1", "--device-bgzf", "1"]}
CLI_SHAPES = [["--tile-sites", "2048", "--devices", "0"], ["--tile-sites", "1000", "--devices", "0"],          # tiles of 1000, 1000, 48
              ["--tile-sites", "1", "--devices", "0"], ["--tile-sites", "1000", "--devices", "0,0"]]              # two contexts of one GPU


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory):
    """2048 sites x 500 samples of phased binary genotypes, gzip-compressed (as test_gpu_cli_input's, at another shape)"""
    import gzip
    gt = synth.binary_sites(0, CLI_S, CLI_N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    path = str(tmp_path_factory.mktemp("inflight") / "in.vcf.gz")
    with gzip.open(path, "wt", compresslevel=1) as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (CLI_S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(CLI_N)) + "\n")
        for i in range(CLI_S):
            idx = (gt[i] & 0xF).astype(np.int64) + 2 * (gt[i] >> 4).astype(np.int64)
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
    return path


@pytest.mark.parametrize("mode", ["b", "z"])
def test_the_program_at_2048_sites_of_500_samples(cli_input, mode, tmp_path):
    """vcfgl_hip in tile mode with GL + PL + DP, the device stages of -O b / -O z at --tile-sites 2048, 1000 and 1 and on two contexts of
    one GPU: the decompressed record stream, the truth file and stdout equal the host twin's (every stage flag 0, one context).  Five
    processes, one at a time, each under a time limit; after one that died nothing more is started"""
    import subprocess
    import cli_stage_cases as sc
    import miscread_util as mu

    def run(name, stage, shape):
        out = str(tmp_path / name)
        argv = [sc.BIN, "-i", cli_input, "-o", out, "-O", mode, "--rng-mode", "0", "--verbose", "1"] + CLI_REF + stage + shape

        def call():
            r = subprocess.run(argv, capture_output=True, text=True, timeout=CLI_TIMEOUT)
            return r.returncode, r.stdout, r.stderr
        t0 = time.perf_counter()
        rc, stdout, stderr = mu.guarded("vcfgl_hip " + " ".join(stage + shape), call)
        print(f"\nvcfgl_hip -O {mode} {' '.join(stage + shape)}: {time.perf_counter() - t0:.2f} s")
        assert rc == 0, (argv, stderr[-1500:])
        return sc.artifacts(out, mode, rc, stdout, stderr)

    twin = run("host", [x for f in sc.STAGES for x in (f, "0")] + ["--records", "1"],
               ["--tile-sites", "4096", "--devices", "0", "--encode-threads", "1", "--threads", "1"])
    assert twin["records"] is not None and twin["truth"] is not None
    if mode == "z":                                          # (the records are there: 2048 lines of 500 columns)
        assert sum(1 for l in twin["records"] if not l.startswith("#")) == CLI_S
    for k, shape in enumerate(CLI_SHAPES):
        dev = run("dev%d" % k, CLI_STAGES[mode], shape)
        assert sc.differences(dev, twin) == [], (mode, shape)
