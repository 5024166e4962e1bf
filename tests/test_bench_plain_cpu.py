"""A plain `bench.py --gpus 1 --steps K --warmup W` run, rehearsed without a GPU (BENCH_TEST_STUB: tests/bench_stub.py stands in for the
device path): one result line whose ms_per_step covers K timed steps, and --dump-outputs writes what the last step computed as float32 /
float64 .npy files -- the same files from run to run."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench

BENCH = os.path.join(ROOT, "bench.py")


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e["BENCH_TEST_STUB"] = "1"
    return e


def _run(*extra):
    return subprocess.run([sys.executable, BENCH, "--gpus", "1", "--sites", "64", "--samples", "8", "--tile-sites", "32"] + list(extra),
                          env=_env(), capture_output=True, text=True, timeout=300)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_prints_the_line_and_dumps_the_last_step(tmp_path):
    dumps = []
    for k in range(2):
        d = str(tmp_path / f"out{k}")
        r = _run("--steps", "3", "--warmup", "2", "--dump-outputs", d)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["warmup"] == 2 and "extra" not in line and "cpu_baseline" not in line
        assert abs(line["value"] - 64 * 8 / (line["ms_per_step"] * 1e-3)) < 1e-4 * line["value"]
        dumps.append(_load(d))
    a, b = dumps
    assert set(a) == {"sites", "site_status", "n_alleles", "alleles2acgt", "fmt_dp", "gl"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    sites = a["sites"].astype(np.int64)
    assert np.array_equal(sites, np.arange(64))                              # 64 sites: all of them
    assert np.array_equal(a["fmt_dp"], np.repeat(sites % 50, 8).reshape(64, 8))   # the stub's depth pattern, row = site
    assert a["gl"].shape == (64, 15, 8) and (a["gl"] == -1.5).all()


def test_dump_of_a_large_output_is_a_fixed_sample(tmp_path):
    import torch
    S, N, G = 5000, 1000, 15
    out = {"site_status": torch.zeros(S, dtype=torch.int32), "fmt_dp": torch.arange(S * N, dtype=torch.int32).reshape(S, N),
           "gl": torch.arange(S, dtype=torch.float32)[:, None, None].expand(S, G, N).contiguous()}
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    sites = a["sites"].astype(np.int64)
    assert 0 < len(sites) <= bench.DUMP_MAX_SITES and np.all(np.diff(sites) > 0) and sites[-1] < S
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["fmt_dp"], (sites[:, None] * N + np.arange(N)).astype(np.float64))
    assert a["gl"].dtype == np.float32 and np.array_equal(a["gl"][:, 0, 0], sites.astype(np.float32))


def test_steps_must_be_positive():
    r = _run("--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr
