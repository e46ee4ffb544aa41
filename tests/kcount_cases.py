"""Counted k-mer sets (`cornetto qv -r`, `cornetto trioeval --pat-reads / --mat-reads`): the rule of include/cornetto_accel.h restated in plain Python —
a `collections.Counter` per channel over kqv_cases.kmers_of, then kqv_cases.query / ktrio_cases.phase on the thresholded sets — the formatter of
what the two commands print, and the cases shared by tests/test_kcount_host.py (the host path, the sim) and tests/test_gpu_kcount.py (the device).
Nothing here touches the library: every expected value comes from the restatement.  The sequences of kqv_cases / ktrio_cases are reused."""
import collections
import functools
import random

import kqv_cases as kc
import ktrio_cases as kt

TILE, RUN, KS = kc.TILE, kc.RUN, kc.KS
CAP, BINS = 65535, 1024
E_ARG, E_NOMEM, E_UNSUPPORTED = -3, -4, -5

# reads: [(channel, [seq])], one entry per batch (and per reads file of the CLI); ms: the thresholds to seal with, a tuple per seal; query: [seq];
# slots: None for a roomy table, else the number of slots
Case = collections.namedtuple("Case", "name channels reads ms query slots")


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
def count(reads, channels, k):
    """-> ([Counter per channel], positions counted)"""
    cnt, n = [collections.Counter() for _ in range(channels)], 0
    for ch, seqs in reads:
        for s in seqs:
            km = kc.kmers_of(s, k)
            n += len(km)
            cnt[ch].update(x for _, x in km)
    return cnt, n


def hist_of(counter):
    h = [0] * BINS
    for c in counter.values():
        h[min(c, CAP, BINS - 1)] += 1
    return h


def solid_of(counter, m):
    return set(x for x, c in counter.items() if min(c, CAP) >= m)


def answer(cnt, m, query, k):
    """-> (solid per channel, the probes' result): (kmers, missing, rows) of kqv_cases.query for one channel, the rows of ktrio_cases.phase for two"""
    S = [solid_of(c, mi) for c, mi in zip(cnt, m)]
    if len(cnt) == 1:
        return (len(S[0]),), kc.query(S[0], query, k)
    return (len(S[0]), len(S[1])), kt.phase(S[0], S[1], query, k)


# ---- the texts ------------------------------------------------------------------------------------------------------------------------------------
def hist_text(hists):
    return "".join("%d\t%s\n" % (c, "\t".join(str(h[c]) for h in hists)) for c in range(1, BINS)).encode()


def expect_qv(read_files, asm_files, k, m):
    """read_files: [[(name, seq)]] per -r file; asm_files: [(path as given, [(name, seq)])] -> dict(stdout, contigs, bed, line, hist, distinct)"""
    recs = [r for f in read_files for r in f]
    cnt, n_pos = count([(0, [s for _, s in recs])], 1, k)
    S = solid_of(cnt[0], m)
    out = ["#file\tcontigs\tbases\tkmers\tmissing\terror\tqv\n"]
    ctab = bed = ""
    for path, rs in asm_files:
        kmers, missing, rows = kc.query(S, [s for _, s in rs], k)
        out.append("%s\t%d\t%d\t%d\t%d\t%s\t%s\n" % ((path, len(rs), sum(len(s) for _, s in rs), sum(kmers), sum(missing)) + kc.qv_strings(sum(kmers), sum(missing), k)))
        ctab = "#contig\tlength\tkmers\tmissing\terror\tqv\n" + "".join(
            "%s\t%d\t%d\t%d\t%s\t%s\n" % ((n, len(s), a, b) + kc.qv_strings(a, b, k)) for (n, s), a, b in zip(rs, kmers, missing))
        bed = "".join("%s\t%d\t%d\n" % (rs[c][0], a, b) for c, a, b in rows)
    line = "[qv] reads: %d records, %d bases, %d k-mers, %d distinct, %d solid (count >= %d), k=%d" % (
        len(recs), sum(len(s) for _, s in recs), n_pos, len(cnt[0]), len(S), m, k)
    return dict(stdout="".join(out).encode(), contigs=ctab.encode(), bed=bed.encode(), line=line.encode(), hist=hist_text([hist_of(cnt[0])]), distinct=len(cnt[0]))


def expect_trio(pat_files, mat_files, asm_files, k, m):
    """pat_files, mat_files: [[(name, seq)]] per reads file; m = (pat, mat) -> dict(stdout, contigs, line, hist, distinct)"""
    cnt, n_pos = count([(0, [s for f in pat_files for _, s in f]), (1, [s for f in mat_files for _, s in f])], 2, k)
    P, M = solid_of(cnt[0], m[0]), solid_of(cnt[1], m[1])
    distinct = len(set(cnt[0]) | set(cnt[1]))
    w = kt.cli_text(pat_files + mat_files, n_pos, distinct, [(path, rs, kt.phase(P, M, [s for _, s in rs], k)) for path, rs in asm_files], k)
    recs = [r for f in pat_files + mat_files for r in f]
    line = "[trioeval] parent reads: %d records, %d bases, %d k-mers, %d distinct, %d pat solid, %d mat solid (count >= %d,%d), k=%d" % (
        len(recs), sum(len(s) for _, s in recs), n_pos, distinct, len(P), len(M), m[0], m[1], k)
    return dict(stdout=w["stdout"], contigs=w["contigs"], line=line.encode(), hist=hist_text([hist_of(cnt[0]), hist_of(cnt[1])]), distinct=distinct)


def fastq(recs):
    return b"".join(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def short_reads(rng, k):
    """400 reads of 150 bases at seeded offsets of a 4 kb sequence, a substitution in every fifth; between them records of 0, 1, k - 1, k, RUN - 1,
    RUN and RUN + 1 bases; invalid bytes at record ends and at the boundaries of the runs a record is dealt in"""
    z = kc.dna(rng, 4000)
    odd = (0, 1, k - 1, k, RUN - 1, RUN, RUN + 1)
    marks = (0, 149, RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, 9 * RUN - 1, 9 * RUN, 150 - k, k - 1)
    out = []
    for i in range(400):
        o = rng.randrange(len(z) - 150)
        r = z[o:o + 150]
        if i % 5 == 0:
            r = kc.sub(r, rng.randrange(150))
        if i % 7 == 3:
            r = kc.put(r, marks[(i // 7) % len(marks)], b"Nn-"[i % 3])
        out.append(r)
        if i % 9 == 4:
            n = odd[(i // 9) % len(odd)]
            o = rng.randrange(len(z) - n)
            r = z[o:o + n]
            if n and (i // 9) % 2:
                r = kc.put(r, (0, n - 1)[(i // 18) % 2], ord("N"))
            out.append(r)
    return z, out


@functools.lru_cache(maxsize=None)
def cases(k):
    """[Case]: every shape at which the counted table can go wrong, for one k"""
    rng = random.Random(3000 + k)
    out = []
    # every case of `qv`, its truth batches counted once, m = 1: today's plain set
    for name, truth, query in kc.cases(k):
        out.append(Case("m1_identity/" + name, 1, [(0, b) for b in truth], [(1,)], query, None))
    # counts add up across records, strands and batches
    y = kc.dna(rng, 2 * TILE + k)
    reads = [(0, [y, y[:TILE + 5]]), (0, [kc.revcomp(y[-300:])])]
    query = [y, kc.sub(y, TILE + 2, 2 * TILE - 100), y[-400:], kc.dna(rng, 500), y[TILE - 50:TILE + 50]]
    out.append(Case("multiplicity", 1, reads, [(1,), (2,), (3,)], query, None))
    # the same reads in a table without a free slot: kept keys sit behind removed ones, an absent key walks the whole table
    out.append(Case("tombstones_at_load_1", 1, reads, [(2,)], query, "distinct"))
    z, rs = short_reads(rng, k)
    out.append(Case("short_reads", 1, [(0, rs[:250]), (0, rs[250:])], [(2,), (1,)], [z, kc.revcomp(z), kc.sub(z, 1000, 2000, 3000)], None))
    # one key above the cap, a second one in the last bin
    out.append(Case("cap_and_last_bin", 1, [(0, [b"A" * (17 * TILE)]), (0, [b"C" * TILE])], [(CAP,), (TILE - k + 1,), (TILE - k + 2,), (1,)],
                    [b"A" * 100, b"C" * 50, b"T" * 40 + b"G" * 40, kc.dna(rng, 200), b"a" * (k - 1) + b"C" * k], None))
    # keys planted with counts 1, 2, 3, 1022, 1023 and 1024: a 40-base unit repeated as separate records
    units = [(c, kc.dna(rng, 40)) for c in (1, 2, 3, 1022, 1023, 1024)]
    recs = [u for c, u in units for _ in range(c)]
    rng.shuffle(recs)
    out.append(Case("hist_bins", 1, [(0, recs[:1500]), (0, recs[1500:])], [(3,), (1023,), (1024,), (1025,)], [b"N".join(u for _, u in units), kc.dna(rng, 100)], None))
    # planted k-mers whose (pat count, mat count) take every pair of {0, 1, 2} x {0, 1, 2}
    s = kc.dna(rng, 9 * 60 + 100)
    pairs = [(a, b) for a in range(3) for b in range(3)]
    rng.shuffle(pairs)
    pat = [s[20 + 60 * i:20 + 60 * i + k] for i, (a, b) in enumerate(pairs) for _ in range(a)]
    mat = [kc.revcomp(s[20 + 60 * i:20 + 60 * i + k]) if i % 2 else s[20 + 60 * i:20 + 60 * i + k] for i, (a, b) in enumerate(pairs) for _ in range(b)]
    out.append(Case("two_channels", 2, [(0, pat[:4]), (1, mat), (0, pat[4:])], [(2, 2), (1, 2), (2, 1), (1, 1)], [s, kc.revcomp(s), s[:300].lower()], None))
    # a mosaic case of `trioeval` with both parents counted twice, m = 2: today's tagged set
    batches, query = next((b, q) for n, b, q in kt.cases(k) if n == "mosaic")
    out.append(Case("mosaic_twice", 2, [(tag - 1, seqs) for tag, seqs in batches] * 2, [(2, 2)], query, None))
    return out


@functools.lru_cache(maxsize=None)
def expected(k):
    """{name: (case, (positions, distinct), [hist per channel], {m: (solid per channel, result)})}: computed once per k and shared"""
    out = {}
    for c in cases(k):
        cnt, n_pos = count(c.reads, c.channels, k)
        distinct = len(set().union(*cnt))
        out[c.name] = (c, (n_pos, distinct), [hist_of(x) for x in cnt], dict((m, answer(cnt, m, c.query, k)) for m in c.ms))
    return out


def slots_of(case, stats):
    return stats[1] if case.slots == "distinct" else 2 * stats[0] + 1
