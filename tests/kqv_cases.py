"""`cornetto qv`: the rule of include/cornetto_accel.h restated in plain Python (a `set` of ints), the formatter of the tables the CLI prints,
and the cases shared by tests/test_kqv_host.py (the host path, the sim) and tests/test_gpu_kqv.py (the device).  Nothing here touches the
library: every expected value comes from the restatement below."""
import math
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"#define CORNETTO_KQV_TILE (\d+)", open(os.path.join(ROOT, "include", "cornetto_accel.h")).read()).group(1))
RUN = TILE // 256          # consecutive bases per thread (csrc/kqv.hpp: KQ_RUN)
KS = (11, 21, 31)
E_UNSUPPORTED, E_NOMEM = -5, -4

CODE = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
def kmers_of(seq, k):
    """(position, canonical k-mer) of every position of `seq` that holds a k-mer"""
    out = []
    mask = (1 << (2 * k)) - 1
    fwd = rc = valid = 0
    for e, b in enumerate(seq):
        c = CODE.get(b)
        if c is None:
            valid = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        valid = min(valid + 1, k)
        if valid == k:
            out.append((e - k + 1, min(fwd, rc)))
    return out


def slow_kmers_of(seq, k):
    """the same from the words of the rule alone, position by position (the check of kmers_of)"""
    out = []
    for i in range(len(seq) - k + 1):
        cs = [CODE.get(b) for b in seq[i:i + k]]
        if None in cs:
            continue
        f = r = 0
        for c in cs:
            f = f << 2 | c
        for c in reversed(cs):
            r = r << 2 | (3 - c)
        out.append((i, min(f, r)))
    return out


def truth_set(contigs, k):
    """-> (S, positions inserted)"""
    S, n = set(), 0
    for s in contigs:
        km = kmers_of(s, k)
        n += len(km)
        S.update(x for _, x in km)
    return S, n


def query(S, contigs, k):
    """-> (kmers[], missing[], rows [(ctg, start, finish)])"""
    kmers, missing, rows = [], [], []
    for c, s in enumerate(contigs):
        km = kmers_of(s, k)
        miss = [i for i, x in km if x not in S]
        kmers.append(len(km))
        missing.append(len(miss))
        cur = None
        for i in miss:
            if cur and i <= cur[2]:          # overlapping or book-ended
                cur[2] = i + k
            else:
                if cur:
                    rows.append(tuple(cur))
                cur = [c, i, i + k]
        if cur:
            rows.append(tuple(cur))
    return kmers, missing, rows


def qv_strings(kmers, missing, k):
    if kmers == 0:
        return "NA", "NA"
    if missing == 0:
        return "0", "inf"
    p = (kmers - missing) / kmers
    e = 1 - math.pow(p, 1.0 / k)
    return "%.3e" % e, "%.2f" % (-10 * math.log10(e))


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------
def expect_cli(truth_files, asm_files, k):
    """truth_files: [[(name, seq)]] per file; asm_files: [(path as given, [(name, seq)])] -> dict(stdout, contigs, bed, truth_line); contigs and bed
    are those of the LAST assembly (the options take one)"""
    recs = [r for f in truth_files for r in f]
    S, n_pos = truth_set([s for _, s in recs], k)
    out = ["#file\tcontigs\tbases\tkmers\tmissing\terror\tqv\n"]
    ctab = bed = ""
    for path, rs in asm_files:
        kmers, missing, rows = query(S, [s for _, s in rs], k)
        out.append("%s\t%d\t%d\t%d\t%d\t%s\t%s\n" % ((path, len(rs), sum(len(s) for _, s in rs), sum(kmers), sum(missing)) + qv_strings(sum(kmers), sum(missing), k)))
        ctab = "#contig\tlength\tkmers\tmissing\terror\tqv\n" + "".join(
            "%s\t%d\t%d\t%d\t%s\t%s\n" % ((n, len(s), a, b) + qv_strings(a, b, k)) for (n, s), a, b in zip(rs, kmers, missing))
        bed = "".join("%s\t%d\t%d\n" % (rs[c][0], a, b) for c, a, b in rows)
    line = "[qv] truth: %d records, %d bases, %d k-mers, %d distinct, k=%d" % (len(recs), sum(len(s) for _, s in recs), n_pos, len(S), k)
    return dict(stdout="".join(out).encode(), contigs=ctab.encode(), bed=bed.encode(), truth_line=line.encode(), distinct=len(S))


def fasta(recs, width=0):
    out = []
    for n, s in recs:
        out.append(b">" + n.encode() + b"\n")
        if width:
            out += [s[i:i + width] + b"\n" for i in range(0, len(s), width)]
        else:
            out.append(s + b"\n")
    return b"".join(out)


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------------
def dna(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def sub(seq, *offsets):
    """a substitution at every offset: the next base of ACGT"""
    s = bytearray(seq)
    for o in offsets:
        s[o] = b"CGTA"[CODE[s[o]]]
    return bytes(s)


def put(seq, o, byte):
    s = bytearray(seq)
    s[o] = byte
    return bytes(s)


def revcomp(seq):
    return seq[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def invalid_offsets(L, k):
    """the offsets the issue names: the contig's ends, the tile seam, and every boundary of a thread's run near them"""
    o = {0, k - 1, L - k, L - 1, TILE - 1, TILE, TILE + k - 2, RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, TILE - RUN - 1, TILE - RUN, TILE + RUN - 1, TILE + RUN}
    return sorted(x for x in o if 0 <= x < L)


def cases(k):
    """[(name, truth batches [[seq]], query [seq])]: every shape at which the kernels can go wrong, for one k"""
    rng = random.Random(1000 + k)
    out = []
    small = [dna(rng, n) for n in (0, 1, k - 1, k, k + 1)]
    out.append(("short_contigs", [small], small + [dna(rng, k + 1), b"", dna(rng, k)]))
    a, b, c = dna(rng, k), dna(rng, 50), dna(rng, k)
    out.append(("k_bases_then_others", [[a, b, c]], [a + b + c, a, b, c, c + a]))
    a = dna(rng, 3 * k)
    b = a[-(k - 1):] + dna(rng, 2 * k)
    out.append(("shared_edge", [[a, b]], [a + b[k - 1:], a, b]))
    L = TILE + 3 * k
    x = dna(rng, L)
    offs = invalid_offsets(L, k)
    out.append(("invalid_in_query", [[x]], [put(x, o, byte) for byte in b"Nn-" for o in offs]))
    xs = [dna(rng, L) for _ in range(3 * len(offs))]
    out.append(("invalid_in_truth", [[put(s, o, byte) for s, (byte, o) in zip(xs, [(byte, o) for byte in b"Nn-" for o in offs])]], xs))
    out.append(("invalid_runs", [[x]], [x[:100] + b"N" * RUN + x[100 + RUN:], x[:TILE - 3] + b"NNNNNN" + x[TILE + 3:], b"N" * L, b"N" * (k - 1) + x[k - 1:]]))
    mixed = bytes(ch + 32 if i % 3 == 0 else ch for i, ch in enumerate(x))
    out.append(("lower_and_mixed_case", [[x[:2000], mixed[2000:]]], [x.lower(), mixed, x]))
    lens = [p + k - 1 for p in (TILE - 1, TILE, TILE + 1, 2 * TILE + k - 1)]
    ts = [dna(rng, n) for n in lens]
    out.append(("tile_lengths", [ts], [sub(s, len(s) // 2) for s in ts] + ts + [sub(s, len(s) - 1) for s in ts]))
    y = dna(rng, 2 * TILE + k)
    out.append(("one_substitution", [[y]], [sub(y, TILE - 1), sub(y, TILE), sub(y, 0), sub(y, len(y) - 1), sub(y, 0, len(y) - 1), sub(y, k - 2), sub(y, len(y) - k + 1)]))
    out.append(("two_substitutions", [[y]], [sub(y, p, p + d) for p in (500, TILE - k, TILE - 1) for d in (k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1)]))
    out.append(("reverse_complement", [[y, x]], [revcomp(y), revcomp(x), revcomp(y.lower())]))
    out.append(("homopolymer", [[b"A" * (3 * TILE)]], [b"A" * (3 * TILE), b"T" * 100, b"C" * 50, b"a" * (TILE + 1) + b"C" + b"t" * TILE]))
    unit = b"ACG"
    s = unit * (2 * TILE // 3)
    out.append(("tandem_repeat", [[s]], [s, sub(s, TILE), (b"AC" * TILE)[:TILE + 7], revcomp(s)]))
    out.append(("two_batches", [[y[:TILE + 100], x], [y[TILE:], b"", x[:k]]], [y, x, sub(y, 77)]))
    return out


def moderate(k):
    """a seeded random truth of 200 kbp in 7 contigs, a query with 1 % substitutions and a few N runs"""
    rng = random.Random(77)
    lens = [60000, 45000, 40001, 30000, 20000, 4096, 903]
    truth = [dna(rng, n) for n in lens]
    q = []
    for s in truth:
        s = sub(s, *rng.sample(range(len(s)), len(s) // 100))
        b = bytearray(s)
        for _ in range(2):
            o, n = rng.randrange(len(b)), rng.randrange(1, 200)
            b[o:o + n] = b"N" * len(b[o:o + n])
        q.append(bytes(b))
    return truth, q
