"""A context gives back what it took: five cycles of create, one asynchronous text tile with a pileup, a fetch-GL request, the
discordance tally and a set-alleles table, one gVCF tile, destroy -- N = 64, max_sites = 256, 32-site tiles -- and the free device
memory (torch.cuda.mem_get_info) after each destroy.  Cycle 1 warms the runtime; the drift is what cycles 3 .. 5 lose against the
reading after cycle 2.

Recorded on e6ba451 (the last commit whose vgl_ctx_destroy freed from hand-kept lists), one MI355X: the reading after every one of
the five destroys was the same number, so PARENT_DRIFT = 0 bytes (this build: 0 too).  The runtime serves small allocations from
2 MiB chunks of its own and the reading moves in whole chunks: hipMalloc of 1024 bytes (max_sites x 4, the smallest plane of this
context that workspace_bytes counts) left it unchanged, the 257th such allocation moved it by 2097152, as did one hipMalloc of
2 MiB -- GRANULE = 2097152 bytes.  A build may drift by less than PARENT_DRIFT + GRANULE.  At that granule this is a guard against
losing a context's large buffers, not a proof of no leak: a small buffer lost once per cycle (a target table, a pinned word, a
plane of a few KiB) stays below it.  The owners' own guard is tests/test_hostmem_cpu.py, under the leak checker.

Also: a context with a tile still in flight destroys cleanly (vgl_ctx_destroy waits for the slot's copies)."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from vcfgl_amd import Simulator, VcfglArgs, _abi

pytestmark = pytest.mark.gpu
N, MAX_SITES, S, CYCLES = 64, 256, 32, 5
PARENT_DRIFT = 0
GRANULE = 2097152


def sim_args():
    a = VcfglArgs(seed=11, depth=3, error_rate=0.05, add_fmt_dp=1, add_pl=1, do_unobserved=2, out_layout=_abi.VGL_LAYOUT_SAMPLE_MAJOR)
    a.rng_mode, a.beta_sampler = _abi.VGL_RNG_TILE, _abi.VGL_BETA_RAND48
    return a


def own_allele_targets(tile):
    """for every site its own first two alleles, swapped: a table the relabelling accepts"""
    nA, a2b = tile.numpy("n_alleles"), tile.numpy("alleles2acgt")
    return [(int(a2b[i][1]), int(a2b[i][0])) if nA[i] >= 2 else (0, 1) for i in range(len(nA))]


def text_tile(sim, gt, keep):
    """site 0 .. S - 1 through vgl_simulate_tile_text_async with a pileup and a fetch-GL request; returns the ticket"""
    lib = sim.lib
    tcap, pcap, fcap = (int(f(sim.ctx, S)) for f in (lib.vgl_ctx_text_bound, lib.vgl_ctx_pileup_bound, lib.vgl_ctx_fetchgl_bound))
    keep.update(vt=np.zeros(tcap, np.uint8), vo=np.zeros(S + 1, np.int64), pt=np.zeros(pcap, np.uint8), po=np.zeros(S + 1, np.int64),
                ft=np.zeros(fcap, np.uint8), fo=np.zeros(S + 1, np.int64), tile=sim.new_tile(S, fields=["fmt_dp", "pl"]))
    keep["pp"] = _abi.PileupTile(keep["pt"].ctypes.data, pcap, keep["po"].ctypes.data, -7)
    keep["fp"] = _abi.FetchGlTile(keep["ft"].ctypes.data, fcap, keep["fo"].ctypes.data, -7)
    sim._check(lib.vgl_ctx_pileup_next(sim.ctx, C.byref(keep["pp"])))
    sim._check(lib.vgl_ctx_fetchgl_next(sim.ctx, C.byref(keep["fp"])))
    t = C.c_int32()
    sim._check(lib.vgl_simulate_tile_text_async(sim.ctx, 0, S, gt.ctypes.data, keep["tile"].byref(), keep["vt"].ctypes.data, tcap,
                                                keep["vo"].ctypes.data, C.byref(t)))
    return t.value


def gvcf_tile(sim, gt, keep):
    lib, G = sim.lib, sim.G
    tcap = int(lib.vgl_ctx_gvcf_text_bound(sim.ctx, S))
    keep.update(items=np.zeros(8 * S, np.int32), gtext=np.zeros(tcap, np.uint8), ro=np.zeros(S + 1, np.int64), bo=np.zeros(S + 1, np.int64),
                fdp=np.zeros(N, np.int32), ldp=np.zeros(N, np.int32), fpl=np.zeros(G * N, np.int32), lpl=np.zeros(G * N, np.int32),
                contig=np.zeros(S, np.int32), pos0=np.arange(S, dtype=np.int64) + S, dps=np.array([1, 3, 5], np.int32),
                gtile=sim.new_tile(S, fields=["fmt_dp"]))
    g = _abi.GvcfTile(keep["items"].ctypes.data, keep["gtext"].ctypes.data, tcap, keep["ro"].ctypes.data, keep["bo"].ctypes.data,
                      keep["fdp"].ctypes.data, keep["fpl"].ctypes.data, keep["ldp"].ctypes.data, keep["lpl"].ctypes.data)
    keep["g"] = g
    t = C.c_int32()
    sim._check(lib.vgl_simulate_tile_gvcf_async(sim.ctx, S, S, gt.ctypes.data, keep["contig"].ctypes.data, keep["pos0"].ctypes.data,
                                                keep["dps"].ctypes.data, 3, keep["gtile"].byref(), C.byref(g), C.byref(t)))
    return t.value


def one_cycle(gt, targets):
    sim = Simulator(sim_args(), N, device=0, max_sites_per_tile=MAX_SITES)
    keep = {}
    sim.discordance(1)
    sim.fetch_gl("AC")
    sim.set_alleles(targets, first_site=0)
    sim._check(sim.lib.vgl_tile_wait(sim.ctx, text_tile(sim, gt, keep)))
    assert keep["vo"][S] > 0 and keep["pp"].text_needed > 0 and keep["fp"].text_needed > 0
    sim.set_alleles(None)
    sim._check(sim.lib.vgl_tile_wait(sim.ctx, gvcf_tile(sim, gt, keep)))
    assert keep["g"].text_needed > 0 and sim.discordance_table().any()
    sim.close()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def free_after_each_cycle():
    gt = synth.acgt_sites(S, N, seed=3, missing=0.02)
    ref = Simulator(sim_args(), N, device=0, max_sites_per_tile=MAX_SITES)
    targets = own_allele_targets(ref.simulate(0, gt))
    ref.close()
    return [one_cycle(gt, targets) for _ in range(CYCLES)]


def test_five_cycles_give_the_memory_back():
    free = free_after_each_cycle()
    drift = free[1] - free[CYCLES - 1]
    print("free device memory after each destroy:", free, "drift from cycle 2 to cycle 5:", drift, "bytes")
    assert drift < PARENT_DRIFT + GRANULE


def test_destroy_with_a_tile_in_flight():
    gt = synth.acgt_sites(S, N, seed=3, missing=0.02)
    sim = Simulator(sim_args(), N, device=0, max_sites_per_tile=MAX_SITES)
    sim.fetch_gl("AC")
    keep = {}
    text_tile(sim, gt, keep)
    assert sim.lib.vgl_ctx_destroy(sim.ctx) == _abi.VGL_OK          # (no vgl_tile_wait: the slot is busy)
    sim.ctx = None
    torch.cuda.synchronize()
    # the device is in order and the caller's arrays were written before the context went away
    assert keep["vo"][S] > 0
    again = Simulator(sim_args(), N, device=0, max_sites_per_tile=MAX_SITES)
    t = again.simulate(0, gt, fields=["fmt_dp"])
    again.close()
    assert np.array_equal(t.numpy("fmt_dp"), keep["tile"].numpy("fmt_dp"))
