"""A numpy model of the records of --depth inf (the reference's simulate_record_true_values, vcfgl.cpp:1089-1262), the yardstick of
vgl_inf.hip and of `vcfgl_hip --device-inf 1`.

Per site: the four bases are counted over the 2 N alleles of the samples and ordered by descending count with an insertion sort that
moves an entry forward only past a strictly smaller count (ties keep A < C < G < T); the record's alleles are the bases that occur
(-doUnobserved 0 / 1 / 2) or all four (3 / 4 / 5) in that order, plus the unobserved allele as the last entry for 1, 2, 4, 5.  Per
sample the true genotype is bcf_alleles2gt of its two bases' positions in that list; it gets GL 0 / GP 1 / PL 0, every other
genotype GL -inf / GP 0 / PL 255.
"""
import numpy as np

SITE_OK = 0
FLOAT_MISSING_BITS = 0x7F800001
INT32_MISSING = -2 ** 31
GL_BITS = (0x00000000, 0xFF800000)          # true genotype, every other one: 0.0f, -inf
GP_BITS = (0x3F800000, 0x00000000)          # 1.0f, 0.0f
PL_VALS = (0, 255)
NO_SITE = 0x7FFFFFFF
LAYOUT_PLANES, LAYOUT_SAMPLE_MAJOR = 0, 1
LETTERS = "ACGT"


def adds_unobserved(do_unobserved):
    return do_unobserved in (1, 2, 4, 5)


def max_alleles(do_unobserved):
    return 5 if adds_unobserved(do_unobserved) else 4


def max_genotypes(do_unobserved):
    a = max_alleles(do_unobserved)
    return a * (a + 1) // 2


def alleles2gt(a, b):
    """bcf_alleles2gt"""
    return b * (b + 1) // 2 + a if b > a else a * (a + 1) // 2 + b


def descending_order(ac):
    """the insertion sort of vcfgl.cpp:1106-1116 over the counts of A, C, G, T"""
    order = [0, 1, 2, 3]
    for i in range(4):
        j = i
        while j > 0 and ac[order[j]] > ac[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    return order


def site_alleles(ac, do_unobserved):
    """(alleles as codes 0 .. 4 with 4 = the unobserved allele, n_alleles_obs) of a site with the allele counts ac[4]"""
    order = descending_order(ac)
    n_obs = sum(1 for c in ac if c > 0)
    alleles = order[:4 if do_unobserved >= 3 else n_obs]
    if adds_unobserved(do_unobserved):
        alleles = alleles + [4]
    return alleles, n_obs


def bad_sites(gt):
    """indices of the sites with a nibble outside 0 .. 3"""
    gt = np.asarray(gt, np.uint8)
    return np.flatnonzero((((gt & 0xF) > 3) | ((gt >> 4) > 3)).any(axis=1))


def fill(gt, do_unobserved, layout=LAYOUT_PLANES):
    """The arrays of a tile from gt (uint8 [n_sites][N], base 0 in the low nibble) as vgl_inf_fill_device leaves them:
    site_status, n_alleles, n_alleles_obs (int32 [n_sites]), alleles2acgt (int8 [n_sites][5]), gl / gp (uint32 bits), pl (int32) and
    pl_u8 (uint8), each [n_sites][G][N] flat in `layout`, `written` (bool, same shape: the elements the call defines -- all of them
    with planes, the first N nG(site) of a slab sample-major) and bad_site.  A bad site's per-sample arrays are unspecified:
    its `written` is False throughout."""
    gt = np.asarray(gt, np.uint8)
    S, N = gt.shape
    G = max_genotypes(do_unobserved)
    out = dict(site_status=np.full(S, SITE_OK, np.int32), n_alleles=np.zeros(S, np.int32), n_alleles_obs=np.zeros(S, np.int32),
               alleles2acgt=np.full((S, 5), -1, np.int8), gl=np.zeros((S, G * N), np.uint32), gp=np.zeros((S, G * N), np.uint32),
               pl=np.zeros((S, G * N), np.int32), pl_u8=np.zeros((S, G * N), np.uint8), written=np.zeros((S, G * N), bool))
    bad = set(int(i) for i in bad_sites(gt))
    out["bad_site"] = min(bad) if bad else NO_SITE
    for i in range(S):
        b0, b1 = (gt[i] & 0xF).astype(int), (gt[i] >> 4).astype(int)
        ac = [int(np.sum(b0 == b) + np.sum(b1 == b)) for b in range(4)]
        alleles, n_obs = site_alleles(ac, do_unobserved)
        nA = len(alleles)
        nG = nA * (nA + 1) // 2
        out["n_alleles"][i], out["n_alleles_obs"][i] = nA, n_obs
        out["alleles2acgt"][i, :nA] = alleles
        if i in bad:
            continue
        tg = np.array([alleles2gt(alleles.index(x), alleles.index(y)) for x, y in zip(b0, b1)])
        hit = np.arange(nG)[:, None] == tg[None, :]                         # [nG][N]
        vals = {"gl": np.where(hit, *GL_BITS), "gp": np.where(hit, *GP_BITS), "pl": np.where(hit, *PL_VALS), "pl_u8": np.where(hit, *PL_VALS)}
        if layout == LAYOUT_PLANES:
            miss = {"gl": FLOAT_MISSING_BITS, "gp": FLOAT_MISSING_BITS, "pl": INT32_MISSING, "pl_u8": 255}
            for k, v in vals.items():
                full = np.full((G, N), miss[k], np.int64)
                full[:nG] = v
                out[k][i] = full.reshape(-1).astype(out[k].dtype)
            out["written"][i] = True
        else:
            for k, v in vals.items():
                out[k][i, :N * nG] = v.T.reshape(-1).astype(out[k].dtype)     # sample s, genotype g at s nG + g
            out["written"][i, :N * nG] = True
    return out


def token(bits_or_value, key):
    """one value as the VCF text writers print it"""
    if key == "PL":
        return str(int(bits_or_value))
    if key == "GL":
        return "0" if bits_or_value == GL_BITS[0] else "-inf"
    return "1" if bits_or_value == GP_BITS[0] else "0"


def record_columns(gt, do_unobserved, keys=("GL", "GP", "PL"), nonref="<*>"):
    """per site (REF, ALT, FORMAT, [sample columns]) as a VCF record of --depth inf shows them"""
    gt = np.asarray(gt, np.uint8)
    m = fill(gt, do_unobserved, LAYOUT_SAMPLE_MAJOR)
    N = gt.shape[1]
    recs = []
    for i in range(gt.shape[0]):
        nA = int(m["n_alleles"][i])
        nG = nA * (nA + 1) // 2
        names = [nonref if a == 4 else LETTERS[a] for a in m["alleles2acgt"][i, :nA]]
        cols = []
        for s in range(N):
            parts = []
            for key in keys:
                arr = m[key.lower()][i, s * nG:(s + 1) * nG]
                parts.append(",".join(token(int(v), key) for v in arr))
            cols.append(":".join(parts) if parts else ".")
        recs.append((names[0], ",".join(names[1:]) if nA > 1 else ".", ":".join(keys) if keys else ".", cols))
    return recs


def read_vcf_gt(path, source=1):
    """The packed true genotypes of a VCF text file's records, [n_records][N] uint8 (0xF: a missing or non-ACGT allele), and their
    (chrom, pos) -- source 1: the GT indices name the record's REF / ALT letters; source 0: index 0 is A, index 1 is C."""
    rows, where = [], []
    for ln in open(path):
        if ln.startswith("#") or not ln.strip():
            continue
        c = ln.rstrip("\n").split("\t")
        names = [c[3]] + ([] if c[4] == "." else c[4].split(","))
        code = [(LETTERS.index(a) if a in LETTERS and len(a) == 1 else 0xF) if source == 1 else k for k, a in enumerate(names)]
        row = []
        for col in c[9:]:
            g = col.split(":")[0].replace("/", "|").split("|")
            b = [code[int(x)] if x.isdigit() and int(x) < len(code) else 0xF for x in g]
            b = (b + [0xF, 0xF])[:2]
            row.append(b[0] | (b[1] << 4))
        rows.append(row)
        where.append((c[0], int(c[1])))
    return np.array(rows, np.uint8), where
