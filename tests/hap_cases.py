"""The haplotype stage of the diploid panel (scripts/create-hapnetto.sh:40-71) restated in plain Python, literally after the script, and the
case generators that test_hap_host.py (the CLI's host path) and test_gpu_hap.py (cornetto_hap_fun on the device) share.  PARITY UNPINNED:
no bedtools here; `merge -d` and `subtract` follow the bedtools manual, the rest the awk one-liners as written.

A haplotype is a list of rows (query name, target index into the assembly, start, end): PAF columns 1, 6, 8, 9.  All arithmetic is integer:
every comparison in the tests is exact."""
import os

import numpy as np

import oracle_bind as ob

D_DEFAULT, F_DEFAULT = 1_000_000, 500      # scripts/create-hapnetto.sh:50, :58
INT32_MAX = 2 ** 31 - 1


def _spans(rows):
    a = np.zeros(len(rows), ob.SPAN_DT)
    if len(rows):
        r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        a["ctg"], a["start"], a["end"] = r[:, 0], r[:, 1], r[:, 2]
    return a


def sort_merge(rows, dist):
    """bedtools sort | bedtools merge -d dist over (ctg, start, end) rows -> list of tuples (the oracle's sequential merge)"""
    if not len(rows):
        return []
    m = ob.ivl_merge(_spans(rows), dist)
    return list(zip(m["ctg"].tolist(), m["start"].tolist(), m["end"].tolist()))


def hap_funbits(lens, rows, D=D_DEFAULT, F=F_DEFAULT):
    """GET_HAP_X_FUN (:40-62) for one haplotype -> (blocks, funbits, number of gaps)"""
    by_query = {}
    for q, c, s, e in rows:
        by_query.setdefault(q, []).append((c, s, e))
    tmp = []
    for q in sorted(by_query):                                   # :48 cut -f 1 | sort -u | while read ctg
        tmp += sort_merge(by_query[q], D)                        # :50 awk '$1==ctg' | bedtools sort | bedtools merge -d 1000000
    tmp2 = []
    on = {}
    for c, s, e in tmp:
        on.setdefault(c, []).append((s, e))
    for c, L in enumerate(lens):                                 # :55 bedtools subtract -a assembly.bed -b tmp.bed
        pos = 0
        for s, e in sorted(on.get(c, [])):
            s, e = min(s, L), min(e, L)
            if s > pos:
                tmp2.append((c, pos, s))
            pos = max(pos, e)
        if pos < L:
            tmp2.append((c, pos, L))
    n_gaps = len(tmp2)
    for c, s, e in tmp:                                          # :58 the awk: both corners of every block, the right one unclamped
        if s >= F:
            tmp2.append((c, s - F, min(s + F, INT32_MAX)))
        if e >= F:
            tmp2.append((c, e - F, min(e + F, INT32_MAX)))
    return tmp, sort_merge(tmp2, 0), n_gaps                              # :61 bedtools sort | bedtools merge


def hap_fun(lens, haps, D=D_DEFAULT, F=F_DEFAULT):
    """hap1_hap2_funbits.bed (:67) for any number of haplotypes -> list of (ctg, start, end) by (ctg, start)"""
    every = []
    for rows in haps:
        every += hap_funbits(lens, rows, D, F)[1]
    return sort_merge(every, 0)


def dip_panel(lens, fun, lowq, haps, D=D_DEFAULT, F=F_DEFAULT, **panel_kw):
    """steps 5-9 (:71-84) with the haplotype funbits joined to the merged windows `fun` and the lowQ rows -> (ctg, start, end) rows"""
    joined = [tuple(r) for r in fun] + hap_fun(lens, haps, D, F)
    out = ob.panel_boring(lens, _spans(joined), _spans(lowq), **panel_kw)
    return list(zip(out["ctg"].tolist(), out["start"].tolist(), out["end"].tolist()))


def bed_text(names, rows):
    return b"".join(b"%s\t%d\t%d\n" % (names[c], s, e) for c, s, e in rows)


def paf_text(names, lens, rows, rng=None, extra=b""):
    """PAF lines of one haplotype: 12 columns, only 1, 6, 8, 9 matter; rows in the given order"""
    out = []
    for q, c, s, e in rows:
        q = q if isinstance(q, bytes) else str(q).encode()
        qs = 0 if rng is None else int(rng.integers(0, 1000))
        out.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60%s\n" % (q, qs + e - s + 7, qs, qs + e - s, b"+-"[(s + e) % 2:][:1], names[c], lens[c], s, e, e - s,
                                                                          e - s, extra))
    return b"".join(out)


def golden_case(golden_dir):
    """tests/golden/hapnetto: names, lens, haps (rows by name resolved to indices), expected funbits and diploid panel"""
    d = os.path.join(golden_dir, "hapnetto")
    names, lens = [], []
    for l in open(os.path.join(d, "asm.bed"), "rb"):
        n, a, b = l.split()
        names.append(n)
        lens.append(int(b) - int(a))
    idx = {n: i for i, n in enumerate(names)}
    haps = []
    for f in ("hap1.paf", "hap2.paf"):
        rows = []
        for l in open(os.path.join(d, f), "rb"):
            t = l.rstrip(b"\n").split(b"\t")
            rows.append((t[0], idx[t[5]], int(t[7]), int(t[8])))
        haps.append(rows)
    def bed(f):
        return [(idx[l.split()[0]], int(l.split()[1]), int(l.split()[2])) for l in open(os.path.join(d, f), "rb")]
    return names, lens, haps, bed("funbits.exp.bed"), bed("dip.exp.bed")


def random_case(seed, lens=None, max_queries=40, DF=None):
    """1-3 haplotypes, 1-40 queries each, 1-12 contigs some of which no row touches; the gaps between the rows of a (query, target) chain are
    drawn around D (D-1, D, D+1), row starts and ends around F (F-1, F, F+1) and at the contig end; D and F are random on odd seeds (or DF)
    -> (lens, haps, D, F) with haps[k] = [(query name, ctg, start, end)] in shuffled order"""
    rng = np.random.default_rng(9000 + seed)
    D, F = D_DEFAULT, F_DEFAULT
    if seed % 2:
        D, F = int(rng.choice([0, 1, 50, 3000, 40_000])), int(rng.choice([1, 2, 63, 500, 801]))
    if DF is not None:
        D, F = DF
    if lens is None:
        n_ctg = int(rng.integers(1, 13))
        lens = [int(rng.integers(2 * F + 2, 6 * D + 20 * F + 1000)) for _ in range(n_ctg)]
        if n_ctg > 2 and seed % 3 == 0:
            lens[int(rng.integers(0, n_ctg))] = 0                   # an empty contig: no gap, no row
        if n_ctg > 1:
            lens[int(rng.integers(0, n_ctg))] = int(rng.integers(1, 2 * F + 2))   # a contig shorter than two flanks
    n_ctg = len(lens)
    usable = [c for c in range(n_ctg) if lens[c] >= 2]
    if not usable:
        lens[0] = 5 * F + 10
        usable = [0]
    touched = [c for c in usable if rng.random() < 0.7] or [usable[0]]
    haps = []
    for k in range(int(rng.integers(1, 4))):
        rows = []
        for q in range(int(rng.integers(1, max_queries + 1))):
            name = b"h%dq%d" % (k + 1, q)
            for c in rng.choice(touched, size=min(len(touched), int(rng.integers(1, 4))), replace=False).tolist():
                L = lens[c]
                s = int(rng.choice([0, max(F - 1, 0), F, F + 1, int(rng.integers(0, L))]))
                for _ in range(int(rng.integers(1, 6))):
                    if s >= L - 1:
                        break
                    e = s + int(rng.choice([1, max(F - 1, 1), F, F + 1, int(rng.integers(1, max(2, L // 3)))]))
                    if s == 0 and rng.random() < 0.3:
                        e = int(rng.choice([max(F - 1, 1), F, F + 1]))
                    if e >= L or rng.random() < 0.1:
                        e = L                                       # ends at the contig end: the right corner reaches beyond it
                    rows.append((name, c, s, e))
                    s = e + int(rng.choice([D - 1, D, D + 1, D + 1, int(rng.integers(-(e - s) // 2, D + 2))]))
                    s = max(s, 0)
        order = rng.permutation(len(rows))
        haps.append([rows[i] for i in order])
    return lens, haps, D, F


def planted_case(n_rows, n_ctg, seed, n_hap=2, queries_per_hap=None, D=20_000, max_len=30_000, F=500):
    """about n_rows rows over n_ctg contigs of a few Mb: many chains per query so that blocks, corners and gaps all run to thousands"""
    rng = np.random.default_rng(77_000 + seed)
    lens = rng.integers(200_000, 8_000_000, size=n_ctg).tolist()
    lens[n_ctg // 2] = 0
    per = n_rows // n_hap
    nq = queries_per_hap or max(1, per // 50)
    haps = []
    for k in range(n_hap):
        q = rng.integers(0, nq, size=per)
        c = rng.integers(0, n_ctg - 1 if n_ctg > 1 else 1, size=per)      # the last contig stays untouched
        c[np.asarray(lens)[c] == 0] = 0
        L = np.asarray(lens)[c]
        s = (rng.random(per) * (L - 1)).astype(np.int64)
        e = np.minimum(s + rng.integers(1, max_len, size=per), L)
        haps.append([(b"h%dq%d" % (k + 1, qi), int(ci), int(si), int(ei)) for qi, ci, si, ei in zip(q.tolist(), c.tolist(), s.tolist(), e.tolist())])
    return lens, haps, D, F


def names_for(lens):
    return [b"ctg%03dl" % i for i in range(len(lens))]


def to_device_rows(haps):
    """rows with query names -> one HAP_ROW_DT array per haplotype (query ids: order of first appearance, per haplotype)"""
    import cornetto_amd
    out = []
    for rows in haps:
        ids = {}
        a = np.zeros(len(rows), cornetto_amd.HAP_ROW_DT)
        for i, (q, c, s, e) in enumerate(rows):
            a[i] = (ids.setdefault(q, len(ids)), c, s, e)
        out.append(a)
    return out
