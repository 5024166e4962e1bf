"""setalleles_hip on the device (vcfgl_amd/csrc/misc/setalfile.hip: BCF input; VCF text is refused there): every byte the device path
writes -- the output file (the decompressed stream for -O b), stderr without the [setalleles] line, the return code -- equals what
--on-device 0 writes (which tests/test_setalhip_cli_cpu.py holds against the model), and `redone on the host` is 0, so the device path
has really done the work.  Also: a record of each PL width and a batch that mixes them, a stop at the first, a middle and the last
record of a batch, and the tie to the simulator (setalleles_hip on the file of a plain run gives the records vcfgl_hip --set-alleles
writes, every field and FORMAT value bit for bit).
Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os
import re
import subprocess

import pytest

import bcf_reader
import sal_file_model as M
from vcfgl_amd import setalleles as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_setalleles")
DATA2 = os.path.join(GOLD, "data", "data2.vcf")
EXT = {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}
TIMEOUT = 120
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started


def _device(path, tsv, prefix, mode="v", **kw):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        rc, so, se = S.set_file(path, tsv, prefix, mode, on_device=True, verbose=True, timeout=TIMEOUT, **kw)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("setalleles_hip ran out of time: no further GPU process is started")
    if rc in (-6, -11, 134, 139, 124, 137):
        _gave_up.append("setalleles_hip")
        pytest.fail("setalleles_hip ended with status %d: no further GPU process is started" % rc)
    return rc, so, se


def _host(path, tsv, prefix, mode="v", **kw):
    return S.set_file(path, tsv, prefix, mode, on_device=False, verbose=True, timeout=TIMEOUT, **kw)


def _counts(stderr):
    m = re.search(r"\[setalleles\] on-device (\d): records (\d+), redone on the host (\d+), bytes sent up (\d+), received (\d+)", stderr)
    assert m, stderr[-2000:]
    return tuple(int(m.group(k)) for k in (2, 3, 4, 5))


def _plain(stderr, prefix):
    return "".join(ln for ln in stderr.splitlines(True) if not ln.startswith("[setalleles]")).replace(prefix, "PREFIX")


def _read(prefix, mode):
    fn = prefix + EXT[mode]
    return M.read_output(fn) if os.path.exists(fn) else None


def _same(tmp_path, path, tsv, mode="v", host=None, **kw):
    """both paths on one file: return code, the output file and stderr must be equal; returns (rc, the host's stderr, the device's)"""
    ph, pd = str(tmp_path / "host"), str(tmp_path / "dev")
    if host is None:
        rh = _host(path, tsv, ph, mode)
        host = (rh[0], _plain(rh[2], ph), _read(ph, mode), rh[2])
    rd = _device(path, tsv, pd, mode, **kw)
    assert rd[0] == host[0], (rd[2][-2000:], host[3][-2000:])
    assert _plain(rd[2], pd) == host[1]
    assert _read(pd, mode) == host[2]
    return host, rd


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sal_shapes")


@pytest.mark.parametrize("mode", ["v", "z"])
def test_text_input_is_refused_on_the_device_before_the_output_is_opened(tmp_path, mode):
    """the text family is worked on the host: --on-device 1 says so and exits 1, there is no quiet fall-back"""
    tsv = os.path.join(GOLD, "data", "data2_alleles1.tsv")
    rc, so, se = _device(DATA2, tsv, str(tmp_path / "dev"), mode)
    assert rc == 1 and "Use --on-device 0" in se and "finished" not in se and _read(str(tmp_path / "dev"), mode) is None


# ---- BCF ------------------------------------------------------------------------------------------------------------------------------
def _write_bcf(tmp_path, name, recs, n_samples, container="bcf"):
    path, tsv = str(tmp_path / (name + "." + container)), str(tmp_path / (name + ".tsv"))
    brecs = M.bcf_records(recs, n_samples, end_every=5)
    M.write_bcf(path, brecs, n_samples, container)
    open(tsv, "w").write(M.tsv_text(recs))
    return path, tsv, brecs


_bfiles = {}


def _bshape(shapes_dir, N, R):
    if (N, R) not in _bfiles:
        recs = M.make_records(N, R, seed=2000 * N + R, wide_pl=True)
        path, tsv, _ = _write_bcf(shapes_dir, "b_n%d_r%d" % (N, R), recs, N, "bcf.gz" if N == 64 else "bcf")
        ph = str(shapes_dir / ("bhost_n%d_r%d" % (N, R)))
        rh = _host(path, tsv, ph, "u")
        _bfiles[(N, R)] = (path, tsv, (rh[0], _plain(rh[2], ph), _read(ph, "u"), rh[2]))
    return _bfiles[(N, R)]


@pytest.mark.parametrize("batch", [1, 7, 4096])
@pytest.mark.parametrize("R", [1, 7, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_bcf_wavefront_workgroup_and_batch_boundaries(tmp_path, shapes_dir, N, R, batch):
    path, tsv, host = _bshape(shapes_dir, N, R)
    assert host[0] == 0, host[3][-2000:]
    _, rd = _same(tmp_path, path, tsv, "u", host=host, batch_records=batch)
    records, redone, up, down = _counts(rd[2])
    assert records == R and redone == 0 and up > 0 and down > 0


@pytest.mark.parametrize("n_old,n_new", [(o, n) for o in range(2, 6) for n in range(2, o + 1)])
def test_bcf_every_pair_of_allele_counts(tmp_path, n_old, n_new):
    recs = M.make_records(67, 9, seed=60 + 10 * n_old + n_new, n_old=n_old, n_new=n_new)
    path, tsv, brecs = _write_bcf(tmp_path, "in", recs, 67)
    host, rd = _same(tmp_path, path, tsv, "b", batch_records=4)
    assert host[0] == 0 and _counts(rd[2])[:2] == (9, 0)
    assert M.read_bcf(str(tmp_path / "dev.bcf"))[1] == M.run_bcf(brecs, [r["target"] for r in recs]).records


@pytest.mark.parametrize("tags", M.TAG_SETS)
@pytest.mark.parametrize("qs", [False, True])
def test_bcf_every_tag_set(tmp_path, tags, qs):
    recs = M.make_records(67, 9, seed=9, tags=tags, qs=qs)
    path, tsv, brecs = _write_bcf(tmp_path, "in", recs, 67, "bcf.gz")
    host, rd = _same(tmp_path, path, tsv, "u", batch_records=4)
    records, redone, up, down = _counts(rd[2])
    assert host[0] == 0 and (records, redone) == (9, 0) and (down > 0) == bool(tags)
    assert M.read_bcf(str(tmp_path / "dev.bcf"))[1] == M.run_bcf(brecs, [r["target"] for r in recs]).records


def test_bcf_a_record_of_each_pl_width_and_a_batch_that_mixes_them(tmp_path):
    recs = M.make_records(70, 12, seed=31, tags="GL:PL", wide_pl=True)
    path, tsv, brecs = _write_bcf(tmp_path, "in", recs, 70)
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    widths = [t for r in want.records for k, t, per in r["fmt"] if k == "PL"]
    assert want.stop is None and set(widths) == {1, 2, 3} and len(set(widths[:4])) > 1       # (one batch of 12 holds all three)
    for batch in (1, 4096):
        host, rd = _same(tmp_path, path, tsv, "u", batch_records=batch)
        body, got = M.read_bcf(str(tmp_path / "dev.bcf"))
        assert host[0] == 0 and _counts(rd[2])[:2] == (12, 0) and got == want.records
        assert body == b"".join(M.encode_record(r, 70) for r in want.records)


@pytest.mark.parametrize("at", [7, 10, 13, 20])
def test_bcf_a_stop_at_the_first_a_middle_and_the_last_record_of_a_batch(tmp_path, at):
    recs = M.make_records(5, 21, seed=78, tags="GL:PL", n_old=3, n_new=2)
    brecs = M.bcf_records(recs, 5)
    k = next(i for i, (key, t, per) in enumerate(brecs[at]["fmt"]) if key == "PL")
    hom_het = [-2000000000, 2000000000, -2000000000, 2000000000, 2000000000, -2000000000]      # any pair of alleles overflows
    brecs[at]["fmt"][k] = ("PL", 3, [list(hom_het) if s == 3 else [0, 1, 2, 3, 4, 5] for s in range(5)])
    path, tsv = str(tmp_path / "in.bcf"), str(tmp_path / "in.tsv")
    M.write_bcf(path, brecs, 5, "bcf")
    open(tsv, "w").write(M.tsv_text(recs))
    want = M.run_bcf(brecs, [r["target"] for r in recs])
    host, rd = _same(tmp_path, path, tsv, "u", batch_records=7)
    assert want.stop == ("pl", recs[at]["pos"]) and len(want.records) == at
    assert host[0] == 1 and "Sample 3 at position %d" % recs[at]["pos"] in host[1] and M.read_bcf(str(tmp_path / "dev.bcf"))[1] == want.records


VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data", "data3.vcf")
SIM = ["--seed", "42", "-e", "0.05", "-d", "3", "-explode", "1", "-doUnobserved", "4", "-addPL", "1", "-addGP", "1", "-addQS", "1", "-O", "u"]


def _vcfgl(out, *flags):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        r = subprocess.run([VCFGL, "-i", DATA3, "-o", out] + SIM + list(flags), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("vcfgl_hip ran out of time: no further GPU process is started")
    if r.returncode in (-6, -11, 134, 139, 124, 137):
        _gave_up.append("vcfgl_hip")
        pytest.fail("vcfgl_hip ended with status %d: no further GPU process is started" % r.returncode)
    assert r.returncode == 0, r.stderr[-2000:]


def test_tie_to_the_simulators_set_alleles(tmp_path):
    """setalleles_hip -O u on the file of a plain run gives the records that the same run with --set-alleles writes: every field, rlen
    included (both write the length of the REF name), and every FORMAT value bit for bit -- the file's floats are the simulated floats"""
    plain, flag, tsv = str(tmp_path / "plain"), str(tmp_path / "flag"), str(tmp_path / "a.tsv")
    _vcfgl(plain)
    recs = list(bcf_reader.Reader(plain + ".bcf").records())
    assert len(recs) >= 5 and all(len(r["alleles"]) == 5 for r in recs)
    with open(tsv, "w") as f:
        for i, r in enumerate(recs):
            t = (r["alleles"][i % 5:] + r["alleles"][:i % 5])[:2 + i % 4]
            f.write(t[0] + "\t" + ",".join(t[1:]) + "\n")
    _vcfgl(flag, "--set-alleles", tsv)
    want = list(bcf_reader.Reader(flag + ".bcf").records())
    host, rd = _same(tmp_path, plain + ".bcf", tsv, "u")
    assert host[0] == 0 and _counts(rd[2])[:2] == (len(recs), 0)
    got = M.read_bcf(str(tmp_path / "dev.bcf"))[1]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g["pos0"], [k for k in g if g[k] != w[k]])
