"""Model of gtdiscordance_hip (vcfgl_amd/csrc/misc) in Python: the rules of the reference's misc/gtDiscordance that the program, its
host path and its kernels must agree with, and the seeded generator of the synthetic truth / call pairs the tests use.

  match     the tool's sequential merge on POS; nSites1 = truth records read so far (1-based)
  GT        two alleles, each '.' or an index; a missing called allele: callmis[i] += 1 and nothing else
  base      the allele's first character through refToInt: Aa0 Cc1 Gg2 Tt3
  GQ        -doGQ 0 none (bin 0); 1-6 the record's GQ; 7 and 8 with a GQ header: the record's GQ, 127 for a record without the tag;
            8 without a GQ header: one allele 127, else the walk over the nG PL values: a missing value is a zero found and puts
            the second best back to 255, 0 is a zero found, a value below the second best replaces it; GQ = min(second best, 127)
  cell      disc_model.classify
  lines     -doGQ 1: nSites1 i dcType GQ; -doGQ 2: nSites1 i dcType refToCallType GQ; -perSite 1: POS i dcType refToCallType
An input the tool asserts on raises Stop(position) -- after the lines of the calls before it.
"""
import gzip
import random
import re

import numpy as np

import disc_model as dm

BASE = {"A": 0, "a": 0, "0": 0, "C": 1, "c": 1, "1": 1, "G": 2, "g": 2, "2": 2, "T": 3, "t": 3, "3": 3}
DC = (0, 1, 0, 1, 1, 1)               # dcType of a cell
CALLTYPE = (1, 1, 2, 2, 3, 4)         # refToCallType of a cell


class Stop(Exception):
    def __init__(self, pos, why):
        Exception.__init__(self, "%s at position %d" % (why, pos))
        self.pos, self.why = pos, why


class Result:
    def __init__(self, n):
        self.table = np.zeros(dm.table_len(n), dtype=np.int64)
        self.listing, self.per_site = [], []
        self.nsites1 = self.nsites2 = 0
        self.stop = None


def read_text(path):
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return raw.decode()


def parse(path):
    header, samples, recs = [], [], []
    for line in read_text(path).split("\n"):
        if not line:
            continue
        if line.startswith("##"):
            header.append(line)
        elif line.startswith("#"):
            samples = line.split("\t")[9:]
        else:
            f = line.split("\t")
            recs.append((int(f[1]), [f[3]] + ([] if f[4] == "." else f[4].split(",")), f[8].split(":"), f[9:]))
    return header, samples, recs


def _gt(tok):
    for sep in "/|":
        if sep in tok:
            a, b = tok.split(sep, 1)
            break
    else:
        return None
    out = []
    for x in (a, b):
        if x == ".":
            out.append(-1)
        elif x.isdigit() and len(x) <= 9:
            out.append(int(x))
        else:
            return None
    return out


def pl_walk(tokens):
    second, zero = 255, False
    for t in tokens:
        if t == ".":
            zero, second = True, 255
        elif int(t) == 0:
            zero = True
        elif int(t) < second:
            second = int(t)
    return min(second, 127), zero


def compare(truth_path, call_path, do_gq=0, per_site=False):
    th, ts, tr = parse(truth_path)
    ch, cs, cr = parse(call_path)
    n = len(ts)
    assert n == len(cs)
    res = Result(n)
    cell, mis, sites = dm.views(res.table, n)
    has_gq = any(h.startswith("##FORMAT=<ID=GQ,") for h in ch)
    ti, nsites1 = 0, 1
    try:
        for pos, alleles, fmt, cols in cr:
            while ti < len(tr) and pos > tr[ti][0]:
                ti += 1
                nsites1 += 1
            if ti >= len(tr) or tr[ti][0] != pos:
                raise Stop(pos, "no truth record")
            tpos, talleles, tfmt, tcols = tr[ti]
            gqi = fmt.index("GQ") if "GQ" in fmt else -1
            pli = fmt.index("PL") if "PL" in fmt else -1
            if do_gq == 0:
                mode = "none"
            elif do_gq <= 6:
                if gqi < 0:
                    raise Stop(pos, "no GQ tag")
                mode = "tag"
            elif do_gq == 7 or has_gq:
                mode = "tag" if gqi >= 0 else "max"
            else:
                if pli < 0 or len(alleles) > 5:
                    raise Stop(pos, "no PL tag or too many alleles")
                mode = "pl"
            res.nsites2 += 1
            if len(cols) != n or len(tcols) != n:
                raise Stop(pos, "sample columns")
            gqs = None
            if mode == "pl" and len(alleles) > 1:
                gqs = []
                for c in cols:
                    f = c.split(":")
                    vals = f[pli].split(",") if pli < len(f) else []
                    if len(vals) != len(alleles) * (len(alleles) + 1) // 2:
                        raise Stop(pos, "PL values")
                    g, zero = pl_walk(vals)
                    if not zero:
                        raise Stop(pos, "no zero PL")
                    gqs.append(g)
            for i in range(n):
                tf, cf = tcols[i].split(":"), cols[i].split(":")
                tg = _gt(tf[tfmt.index("GT")]) if tfmt.index("GT") < len(tf) else None
                cg = _gt(cf[fmt.index("GT")]) if fmt.index("GT") < len(cf) else None
                if tg is None or cg is None:
                    raise Stop(pos, "not diploid")
                if -1 in tg:
                    raise Stop(pos, "true genotype missing")
                if -1 in cg:
                    mis[i] += 1
                    continue
                try:
                    tb = [BASE[talleles[a][0]] for a in tg]
                    cb = [BASE[alleles[a][0]] for a in cg]
                except (KeyError, IndexError):
                    raise Stop(pos, "allele")
                if mode == "none":
                    gq = 0
                elif mode == "max" or (mode == "pl" and gqs is None):
                    gq = 127
                elif mode == "pl":
                    gq = gqs[i]
                else:
                    tok = cf[gqi] if gqi < len(cf) else "."
                    gq = int(tok) if tok.lstrip("-").isdigit() else 0
                if mode != "none" and not 1 <= gq <= 127:
                    raise Stop(pos, "GQ")
                c = int(dm.classify(np.array(tb[:1]), np.array(tb[1:]), np.array(cb[:1]), np.array(cb[1:]))[0])
                cell[i, c, gq] += 1
                if do_gq == 1:
                    res.listing.append("%d\t%d\t%d\t%d\n" % (nsites1, i, DC[c], gq))
                elif do_gq == 2:
                    res.listing.append("%d\t%d\t%d\t%d\t%d\n" % (nsites1, i, DC[c], CALLTYPE[c], gq))
                if per_site:
                    res.per_site.append("%d\t%d\t%d\t%d\n" % (pos, i, DC[c], CALLTYPE[c]))
    except Stop as e:
        res.stop = e
        return res
    if tr:
        nsites1 += len(tr) - 1 - ti
    res.nsites1 = nsites1
    sites[0], sites[1] = res.nsites2, nsites1 - res.nsites2
    return res


def table_from_listing(text, n, mode):
    """the lines of -doGQ 2 summed back into a table (cells of hom->hom and het->het by dcType)"""
    table = np.zeros(dm.table_len(n), dtype=np.int64)
    cell, _, _ = dm.views(table, n)
    back = {(1, 0): 0, (1, 1): 1, (2, 0): 2, (2, 1): 3, (3, 1): 4, (4, 1): 5}
    for line in text.split("\n"):
        if line:
            f = [int(x) for x in line.split("\t")]
            assert mode == 2
            cell[f[1], back[(f[3], f[2])], f[4]] += 1
    return table


def summary(stderr):
    """the three counts of the program's stderr summary"""
    out = []
    for key in ("Number of sites in truth file: ", "Number of sites in the truth file not in the call file: ", "Number of sites used in comparison: "):
        at = stderr.index(key) + len(key)
        out.append(int(stderr[at:stderr.index("\n", at)]))
    return tuple(out)


# ---- synthetic pairs ----------------------------------------------------------------------------------------------------------------
FORMATS = ("GT:GQ", "GT:DP:GQ", "GT:PL:GQ", "GT:GQ:PL", "GT:PL")
WIDE = ["A", "C", "G", "T", "AC", "CA", "GT", "TG", "AAC", "CCA", "GGT", "TTG"]          # 12 alleles: indices of two digits


def write_pair(truth_path, call_path, n, n_records, fmt, seed, first_pos=8, invariant=True, odd_share=0.0, wide=True):
    """A truth file and a call file of `n` samples.  About a fifth more truth records than call records; both phase characters;
    missing calls; records of 12 alleles (two-digit indices) where `wide` and the FORMAT has a GQ; invariant call records (ALT '.',
    FORMAT GT alone where the FORMAT has a GQ) where `invariant`; about `odd_share` of the call records carry one token outside the device grammar (an allele
    index of three digits) that the host rules read."""
    rnd = random.Random(seed)
    has_gq = "GQ" in fmt.split(":")
    head = ["##fileformat=VCFv4.2", "##contig=<ID=chr1,length=4294967295>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']
    chead = list(head) + ['##FORMAT=<ID=DP,Number=1,Type=Integer,Description="d">']
    if has_gq:
        chead.append('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">')
    if "PL" in fmt.split(":"):
        chead.append('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p">')
    names = "\t".join("ind%d" % i for i in range(n))
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + names
    tl, cl = head + [cols], chead + [cols]
    pos = first_pos
    written = 0
    while written < n_records:
        pos += 1
        in_call = rnd.random() < 0.8
        kind = rnd.random()
        if invariant and kind < 0.15:
            alleles = [rnd.choice("ACGT")]
        elif wide and has_gq and kind < 0.3:
            alleles = list(WIDE)
            rnd.shuffle(alleles)
        else:
            alleles = rnd.sample("ACGT", rnd.randint(2, 4))
        nA = len(alleles)
        tg = []
        for i in range(n):
            a = rnd.randrange(nA)
            b = a if rnd.random() < 0.5 else rnd.randrange(nA)
            tg.append("%d%s%d" % (a, rnd.choice("/|"), b))
        tl.append("chr1\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s" % (pos, alleles[0], ",".join(alleles[1:]) or ".", "\t".join(tg)))
        if not in_call:
            continue
        written += 1
        # the call file lists its alleles in an order of its own: the comparison goes through the bases
        calleles = list(alleles)
        rnd.shuffle(calleles)
        keys = ["GT"] if nA == 1 and has_gq else fmt.split(":")      # (-doGQ 8 without a GQ header reads PL of every record)
        nG = nA * (nA + 1) // 2
        odd_at = rnd.randrange(n) if rnd.random() < odd_share else -1
        cc = []
        for i in range(n):
            t = [alleles[int(x)] for x in tg[i].replace("|", "/").split("/")]
            if rnd.random() < 0.1:
                a, b = rnd.choice(((-1, -1), (-1, 0), (0, -1)))
            elif rnd.random() < 0.6:
                a, b = calleles.index(t[0]), calleles.index(t[1])
                if rnd.random() < 0.5:
                    a, b = b, a
            else:
                a, b = rnd.randrange(nA), rnd.randrange(nA)
            form = "%03d" if i == odd_at else rnd.choice(("%d", "%d", "%02d"))
            gt = rnd.choice("/|").join("." if x < 0 else form % x for x in (a, b))
            vals = []
            for k in keys:
                if k == "GT":
                    vals.append(gt)
                elif k == "DP":
                    vals.append(str(rnd.randint(0, 40)))
                elif k == "GQ":
                    vals.append("." if a < 0 or b < 0 else str(rnd.choice((1, 2, 9, 10, 99, 100, 126, 127, rnd.randint(1, 127)))))
                elif k == "PL":
                    if nA > 5:
                        vals.append(".")
                    elif a < 0 or b < 0:
                        vals.append(",".join(["."] * nG))
                    else:
                        p = [rnd.choice((0, 3, 3, 17, 126, 127, 128, 255, 1000, rnd.randint(1, 300))) for _ in range(nG)]
                        p[rnd.randrange(nG)] = 0 if rnd.random() < 0.9 else "."
                        vals.append(",".join(str(x) for x in p))
            cc.append(":".join(vals))
        cl.append("chr1\t%d\t.\t%s\t%s\t50\tPASS\t.\t%s\t%s" % (pos, calleles[0], ",".join(calleles[1:]) or ".", ":".join(keys), "\t".join(cc)))
    for _ in range(rnd.randint(0, 3)):                     # truth records behind the last call record
        pos += 1
        tl.append("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t%s" % (pos, "\t".join(["0/1"] * n)))
    with open(truth_path, "w") as f:
        f.write("\n".join(tl) + "\n")
    with open(call_path, "w") as f:
        f.write("\n".join(cl) + "\n")


# ---- the PLAIN grammar (vcfgl_amd/csrc/misc/gtdisc_core.h): what the device accepts; None = the record goes to the host rules ----
GQ_NONE, GQ_TAG, GQ_MAX, GQ_PL = range(4)
_PLAIN_GT = re.compile(r"(\.|[0-9]{1,2})[/|](\.|[0-9]{1,2})")


def _nibble(amap, a):
    return (amap >> (4 * a)) & 15


def _plain_gt(column, gti):
    f = column.split(":")
    m = _PLAIN_GT.fullmatch(f[gti]) if gti < len(f) else None
    return None if m is None else [-1 if x == "." else int(x) for x in m.groups()]


def plain_true(text, gti, nal, amap):
    """the truth column at the start of `text` (it ends at a tab or at the text's end) -> the byte of its bases, or None"""
    g = _plain_gt(text.split("\t")[0], gti)
    if g is None or -1 in g or max(g) >= min(nal, 16):
        return None
    b = [_nibble(amap, a) for a in g]
    return None if max(b) > 3 else b[0] | b[1] << 4


def plain_call(text, gti, gqi, pli, nal, amap, gq_mode):
    """the call column at the start of `text` -> (byte of its bases or 0xFF, GQ), or None"""
    column = text.split("\t")[0]
    f = column.split(":")
    g = _plain_gt(column, gti)
    if g is None:
        return None
    gq = 0
    if gq_mode == GQ_PL and nal > 1:
        vals = f[pli].split(",") if pli < len(f) else []
        if len(vals) != nal * (nal + 1) // 2 or not all(re.fullmatch(r"\.|[0-9]{1,4}", v) for v in vals):
            return None
        gq, zero = pl_walk(vals)
        if not zero:
            return None
    elif gq_mode in (GQ_PL, GQ_MAX):
        gq = 127
    if -1 in g:
        return 0xFF, 0
    if max(g) >= min(nal, 16):
        return None
    b = [_nibble(amap, a) for a in g]
    if max(b) > 3:
        return None
    if gq_mode == GQ_TAG:
        if gqi >= len(f) or not re.fullmatch(r"[0-9]{1,3}", f[gqi]) or not 1 <= int(f[gqi]) <= 127:
            return None
        gq = int(f[gqi])
    return b[0] | b[1] << 4, gq


def plain_record(truth, call, n, t, c, gq_mode):
    """a record of two regions by the plain grammar: the three planes, or None.  t = (gti, nal, amap), c = (gti, gqi, pli, nal, amap)"""
    tc, cc = truth.split("\t"), call.split("\t")
    tb = [plain_true(x, *t) for x in tc[:n]]
    if None in tb or len(tc) != n:
        return None
    cb = [plain_call(x, *c, gq_mode) for x in cc[:n]]
    if None in cb or len(cc) != n:
        return None
    return tb + [x[0] for x in cb] + [x[1] for x in cb]
