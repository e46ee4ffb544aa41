"""k-mer completeness and copy-number spectrum (`cornetto qv -r ... --completeness --spectra-cn FILE`): the rule of include/cornetto_accel.h restated
in plain Python — two `collections.Counter` over kqv_cases.kmers_of, one of the reads and one of the assembly, the 6 x 1024 spectrum of the two,
solid and found for a threshold — the two texts the CLI prints, and the cases shared by tests/test_kspec_host.py (the host path, the sim) and
tests/test_gpu_kspec.py (the device).  Nothing here touches the library: every expected value comes from the restatement."""
import collections
import functools
import random

import kcount_cases as cc
import kqv_cases as kc

TILE, RUN, KS = kc.TILE, kc.RUN, kc.KS
CAP, BINS, CN = cc.CAP, cc.BINS, 6
E_ARG, E_NOMEM, E_UNSUPPORTED = cc.E_ARG, cc.E_NOMEM, cc.E_UNSUPPORTED
PLANTED_MS = (1, 2, 3, 1023, 1024, 1025)

# reads: [[seq]], a batch (a kset_count call, a -r file) each; asm: [[seq]], a batch (a kset_copies call) each; ms: the thresholds to take solid and
# found at; slots: None for a roomy table, "union" for exactly the distinct keys of reads and assembly together, or a number
Case = collections.namedtuple("Case", "name reads asm ms slots")


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
def counter(batches, k):
    """-> (Counter of the canonical k-mers, positions)"""
    cnt, n = collections.Counter(), 0
    for b in batches:
        for s in b:
            km = kc.kmers_of(s, k)
            n += len(km)
            cnt.update(x for _, x in km)
    return cnt, n


def spectrum(R, A):
    """spec[a][c] = keys with min(copies, 5) == a and min(count, 1023) == c, over the keys that are in the reads or in the assembly"""
    spec = [[0] * BINS for _ in range(CN)]
    for x in set(R) | set(A):
        spec[min(A[x], CN - 1)][min(R[x], CAP, BINS - 1)] += 1
    return spec


def totals(R, A, m):
    """-> (solid, found)"""
    S = [x for x, c in R.items() if min(c, CAP) >= m]
    return len(S), sum(1 for x in S if A[x] >= 1)


def completeness(solid, found):
    return "%.6f" % (found / solid) if solid else "NA"


# ---- the texts ------------------------------------------------------------------------------------------------------------------------------------
def spectra_text(spec):
    return ("#count\tcn0\tcn1\tcn2\tcn3\tcn4\tcn5+\n" + "".join("%d\t%s\n" % (c, "\t".join(str(spec[a][c]) for a in range(CN))) for c in range(BINS))).encode()


def expect_qv(read_files, asm_files, k, m):
    """kcount_cases.expect_qv with --completeness: the three columns behind every row; `spectra`: the --spectra-cn text of the LAST assembly"""
    w = cc.expect_qv(read_files, asm_files, k, m)
    R, _ = counter([[s for f in read_files for _, s in f]], k)
    rows = w["stdout"].decode().split("\n")
    out = [rows[0] + "\tsolid\tfound\tcompleteness"]
    spec = None
    for row, (path, rs) in zip(rows[1:], asm_files):
        A, _ = counter([[s for _, s in rs]], k)
        solid, found = totals(R, A, m)
        out.append("%s\t%d\t%d\t%s" % (row, solid, found, completeness(solid, found)))
        spec = spectrum(R, A)
    w["plain"] = w["stdout"]
    w["stdout"] = ("\n".join(out) + "\n").encode()
    w["spectra"] = spectra_text(spec)
    w["union"] = len(set(R) | set(A))
    return w


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def planted(rng):
    """40-base units with read counts 0 (absent), 1, 2, 3, 1022, 1023, 1024 — three units a low class, two a high one — planted 0 to 6 times in an
    assembly of four contigs, every other occurrence reverse-complemented, an N between units -> (reads [seq], contigs [seq], [(count, copies)])"""
    plan, reads, pieces = [], [], []
    for i, c in enumerate((0, 1, 2, 3, 1022, 1023, 1024)):
        for j in range(3 if c < 1000 else 2):
            a = (2 * i + 3 * j + (1 if c == 0 else 0)) % 7
            u = kc.dna(rng, 40)
            plan.append((c, a))
            reads += [u] * c
            pieces += [u if t % 2 == 0 else kc.revcomp(u) for t in range(a)]
    rng.shuffle(reads)
    rng.shuffle(pieces)
    return reads, [b"N".join(pieces[i::4]) for i in range(4)], plan


def seams(rng, k):
    """one contig of 2 * TILE + k bases with invalid bytes and lowercase stretches at run and tile boundaries, and contigs of 0, 1, k - 1, k, RUN - 1,
    RUN and RUN + 1 bases"""
    L = 2 * TILE + k
    y = bytearray(kc.dna(rng, L))
    for o in (RUN - 3, TILE - 5, TILE + RUN - 2, 2 * TILE - 4):
        y[o:o + 9] = bytes(y[o:o + 9]).lower()
    for i, o in enumerate(kc.invalid_offsets(L, k)):
        y[o] = b"Nn-"[i % 3]
    return [bytes(y)] + [kc.dna(rng, n) for n in (0, 1, k - 1, k, RUN - 1, RUN, RUN + 1)]


@functools.lru_cache(maxsize=None)
def cases(k):
    rng = random.Random(4000 + k)
    out = []
    reads, contigs, plan = planted(rng)
    half = len(reads) // 2
    out.append(Case("planted", [reads[:half], reads[half:]], [contigs], PLANTED_MS, None))
    # the same contigs handed over in two calls and in reverse order: the same spectrum (test_*: compared with `planted`)
    out.append(Case("batches/two", [reads], [contigs[:1], contigs[1:]], PLANTED_MS, None))
    out.append(Case("batches/reversed", [reads], [contigs[::-1]], PLANTED_MS, None))
    s = seams(rng, k)
    out.append(Case("seams", [s + s], [s], (1, 2, 3), None))
    out.append(Case("one_key", [[b"A" * 100]], [[b"A" * (TILE + 7)]], (1, 100 - k + 1, 100 - k + 2), None))
    out.append(Case("one_key/one_slot", [[b"A" * 100]], [[b"A" * (TILE + 7)]], (1,), 1))
    mult = next(c for c in cc.cases(k) if c.name == "multiplicity")
    out.append(Case("neighbours_at_load_1", [b for _, b in mult.reads], [mult.query], (1, 2, 3), "union"))
    return out


@functools.lru_cache(maxsize=None)
def second_assembly(k):
    """`two_assemblies`: B for the reads of `planted` — two of A's contigs in the other order, and a novel one"""
    case = cases(k)[0]
    rng = random.Random(4100 + k)
    return [[case.asm[0][2], kc.dna(rng, 300), case.asm[0][0]]]


Exp = collections.namedtuple("Exp", "case stats hist spec totals union asm_positions")


@functools.lru_cache(maxsize=None)
def expected(k):
    """{name: Exp(case, (positions, distinct) of the reads, hist, spec, {m: (solid, found)}, distinct keys of reads and assembly, positions of the
    assembly)}: computed once per k and shared"""
    out = {}
    for c in cases(k):
        R, n_pos = counter(c.reads, k)
        A, a_pos = counter(c.asm, k)
        out[c.name] = Exp(c, (n_pos, len(R)), cc.hist_of(R), spectrum(R, A), dict((m, totals(R, A, m)) for m in c.ms), len(set(R) | set(A)), a_pos)
    return out


def slots_of(e):
    if e.case.slots == "union":
        return e.union
    return e.case.slots or 2 * (e.stats[0] + e.asm_positions) + 1
