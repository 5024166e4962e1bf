"""VGL_RNG_TILE on the device against the EXACT laws of the reference's samplers: the cases of tests/test_tile_laws_cpu.py
(law_cases.py, statistics of laws.py) at 1e6 evaluations per case instead of 1e5 -- tile mode is what every throughput figure is
measured in, and no reference program produces its values; what ties it to the reference is that its draws follow the reference's
distributions and are independent between samples, sites, reads and streams.  Read-level cases (per-read dumps) stay at 1.3e5
evaluations so that a case's host arrays stay below 100 MB.  The negative controls live in the CPU file: device and oracle agree
bit for bit under caller layouts (tests/test_gpu_caller_layouts.py).

Limits are conditions, not measurements: |z| < 5, chi-square < chi2_limit(dof); seeds are 1000 + the case's index in
law_cases.CASES, fixed before the first run.

Observed on an MI355X (87 statistics: 60 z, 22 chi-square, 5 exact counts), every case at its first seed; the oracle, run at these
shapes beforehand, gave the same figures to the last printed digit:
  worst |z|                 2.32   (depth-5: variance)
  worst chi-square / limit  0.70   (read-errp-0.2-0.032: histogram of u)"""
import pytest

import law_cases as lc
from vcfgl_amd import Simulator

pytestmark = pytest.mark.gpu

# (sites, samples) per kind of case
SHAPE = {"depth": (4096, 256), "depths": (4096, 252), "haplotype": (4096, 256), "base": (512, 256), "errp": (512, 256), "site": (20000, 1),
         "tail": (200000, 1), "independence": (512, 256)}


def run(args, gt, site0=0, fields=None, read_capacity=0, deviates=False):
    sim = Simulator(args, gt.shape[1], device=0, max_sites_per_tile=gt.shape[0])
    t = sim.simulate(site0, gt, fields=fields, read_capacity=read_capacity, deviates=deviates)
    sim.close()
    return t


@pytest.mark.parametrize("name,kind,param", lc.POSITIVE, ids=[c[0] for c in lc.POSITIVE])
def test_device_tile_mode_follows_the_exact_law(name, kind, param):
    S, N = SHAPE[kind]
    if name == "read-errp-0.01-1e-09":
        S = 192                                                    # shape parameters of 1e5 and 1e7: the continued fraction of F takes thousands of terms
    lc.assert_inside(name, lc.run_case(run, name, kind, param, S, N))
