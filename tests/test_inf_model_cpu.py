"""The numpy model of --depth inf records (tests/inf_model.py) against what the reference program wrote: the golden test4.vcf (its
allele lists and every GL / GP / PL token), and the multi-allelic input data5, whose first site ties G and T at 3 alleles each."""
import os

import numpy as np
import pytest

import golden_util as gu
import inf_model as im

TEST4 = os.path.join(gu.REFVCF, "reference", "test4", "test4.vcf")
TEST4_TRUTH = os.path.join(gu.REFVCF, "reference", "test4", "test4.truth.vcf")
DATA5 = os.path.join(gu.REFVCF, "data", "data5_acgt_multiallelic.vcf")


def record_lines(path):
    return [ln.rstrip("\n").split("\t") for ln in open(path) if not ln.startswith("#") and ln.strip()]


def test_the_model_reproduces_the_reference_test4_records():
    # the truth file holds the genotypes of every site the run wrote, exploded ones included, with the binary alleles spelled A, C
    gt, where = im.read_vcf_gt(TEST4_TRUTH, source=1)
    want = record_lines(TEST4)
    assert len(want) == len(where) == 10 and gt.shape == (10, 2)
    got = im.record_columns(gt, do_unobserved=1, keys=("GL", "GP", "PL"), nonref="<*>")
    for (chrom, pos), (ref, alt, fmt, cols), w in zip(where, got, want):
        assert [chrom, str(pos), ref, alt, fmt] + cols == [w[0], w[1], w[3], w[4], w[8]] + w[9:], (chrom, pos)
    assert {w[4] for w in want} == {"<*>", "C,<*>"} and want[5][3] == "C"          # (one allele, two alleles, and a site without A)


def test_ties_keep_acgt_order_on_data5():
    gt, where = im.read_vcf_gt(DATA5, source=1)
    assert where[0] == ("chr22", 2) and gt.shape == (6, 4)
    # site 1: C T,G with 2|2 0|0 1|1 1|2 -> C 2, G 3, T 3: the tie keeps G before T
    lists = {d: [im.record_columns(gt, d, keys=("PL",), nonref="<*>" if d in (1, 4) else "<NON_REF>")[i][:2] for i in range(6)] for d in range(6)}
    assert lists[0][0] == ("G", "T,C") and lists[1][0] == ("G", "T,C,<*>") and lists[2][0] == ("G", "T,C,<NON_REF>")
    assert lists[3][0] == ("G", "T,C,A") and lists[4][0] == ("G", "T,C,A,<*>") and lists[5][0] == ("G", "T,C,A,<NON_REF>")
    # site 2: G T,A,C with 0|0 0|0 0|0 1|0 -> G 7, T 1; site 3: all C; sites 4, 5: all G, all C; site 6: all T
    assert lists[0] == [("G", "T,C"), ("G", "T"), ("C", "."), ("G", "."), ("C", "."), ("T", ".")]
    assert lists[3][2] == ("C", "A,G,T") and lists[4][5] == ("T", "A,C,G,<*>")        # (unobserved bases follow in A < C < G < T order)
    # the last sample of site 1 is T|G: alleles G, T, C -> indices 1, 0 -> genotype 1
    cols = im.record_columns(gt, 0, keys=("GL", "GP", "PL"))[0][3]
    assert cols[3] == "-inf,0,-inf,-inf,-inf,-inf:0,1,0,0,0,0:255,0,255,255,255,255"
    assert cols[0] == "0,-inf,-inf,-inf,-inf,-inf:1,0,0,0,0,0:0,255,255,255,255,255"       # G|G
    assert cols[1].split(":")[2] == "255,255,255,255,255,0"                                # C|C: allele 2 -> genotype 5


@pytest.mark.parametrize("ac,order", [([1, 2, 2, 2], [1, 2, 3, 0]), ([2, 2, 2, 2], [0, 1, 2, 3]), ([0, 0, 0, 4], [3, 0, 1, 2]), ([1, 3, 1, 3], [1, 3, 0, 2]),
                                      ([0, 1, 0, 1], [1, 3, 0, 2]), ([3, 2, 1, 0], [0, 1, 2, 3]), ([0, 1, 2, 3], [3, 2, 1, 0])])
def test_descending_order_is_a_stable_sort(ac, order):
    assert im.descending_order(ac) == order == sorted(range(4), key=lambda b: (-ac[b], b))


def test_layouts_and_missing_values():
    gt = np.array([[0x00, 0x10, 0x01], [0x22, 0x22, 0x22], [0x30, 0xF0, 0x21]], np.uint8)
    p = im.fill(gt, 1, im.LAYOUT_PLANES)
    s = im.fill(gt, 1, im.LAYOUT_SAMPLE_MAJOR)
    assert p["bad_site"] == s["bad_site"] == 2 and list(p["n_alleles"][:2]) == [3, 2] and list(p["n_alleles_obs"][:2]) == [2, 1]
    assert p["alleles2acgt"][:2].tolist() == [[0, 1, 4, -1, -1], [2, 4, -1, -1, -1]]
    N, G = 3, 15
    pl = p["pl"].reshape(3, G, N)
    assert pl[0, :6].T.tolist() == [[0, 255, 255, 255, 255, 255], [255, 0, 255, 255, 255, 255], [255, 0, 255, 255, 255, 255]]      # hets in both nibble orders
    assert (pl[0, 6:] == im.INT32_MISSING).all() and (p["gl"].reshape(3, G, N)[1, 3:] == im.FLOAT_MISSING_BITS).all() and p["written"][:2].all()
    assert s["pl"][0, :18].reshape(3, 6).tolist() == pl[0, :6].T.tolist() and s["written"][0].sum() == 18 and s["written"][1].sum() == 9
    assert not p["written"][2].any() and not s["written"][2].any()
