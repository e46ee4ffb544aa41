"""`cornetto trioeval`: the rule of include/cornetto_accel.h restated in plain Python (two `set`s of ints from kqv_cases.kmers_of and a loop over
the positions), the formatter of the tables the CLI prints, and the cases shared by tests/test_ktrio_host.py (the host path, the sim) and
tests/test_gpu_ktrio.py (the device).  Nothing here touches the library: every expected value comes from the restatement below.

Two constructions.  `mosaic`: a random base sequence B, pat and mat are B with substitutions at chosen offsets, the assembly is a mosaic of
stretches taken from either parent — every heterozygous site gives a run of up to k markers.  `plant`: the assembly is a random sequence, the
parents are the k-mers at chosen positions of it (a parental contig of k bases each), so a marker of a chosen type stands at exactly a chosen
position — at a word seam, a tile seam, the last position.  A planted case states its markers, and cases() checks the statement with the
restatement (for k = 11 a random 11-mer recurs now and then: the builder moves on to the next seed until the statement holds)."""
import functools
import random

import kqv_cases as kc

TILE, KS = kc.TILE, kc.KS
PAT, MAT = 1, 2
E_ARG, E_NOMEM, E_UNSUPPORTED = -3, -4, -5
NAMES = ("kmers", "pat", "mat", "pp", "pm", "mp", "mm")


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
def parent_sets(batches, k):
    """batches: [(tag, [seq])] -> (P, M, positions inserted)"""
    sets, n = {PAT: set(), MAT: set()}, 0
    for tag, seqs in batches:
        for s in seqs:
            km = kc.kmers_of(s, k)
            n += len(km)
            sets[tag].update(x for _, x in km)
    return sets[PAT], sets[MAT], n


def markers(P, M, seq, k):
    """-> (positions that hold a k-mer, [(position, type)] of the markers in order)"""
    km = kc.kmers_of(seq, k)
    return len(km), [(i, PAT if x in P else MAT) for i, x in km if (x in P) != (x in M)]


def phase(P, M, contigs, k):
    """-> [[kmers, pat, mat, pp, pm, mp, mm]] per contig"""
    out = []
    for s in contigs:
        n, ms = markers(P, M, s, k)
        c = [n, 0, 0, 0, 0, 0, 0]
        prev = 0
        for _, t in ms:
            c[t] += 1
            if prev:
                c[3 + (prev - 1) * 2 + (t - 1)] += 1
            prev = t
        out.append(c)
    return out


def totals(rows):
    """-> (kmers, pat, mat, pairs, switches, hamming) of an assembly"""
    return (sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows), sum(sum(r[3:]) for r in rows), sum(r[4] + r[5] for r in rows),
            sum(min(r[1], r[2]) for r in rows))


def rate(a, b):
    return "NA" if b == 0 else "%.6f" % (a / b)


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------
def expect_cli(pat_files, mat_files, asm_files, k, known=None):
    """pat_files, mat_files: [[(name, seq)]] per file; asm_files: [(path as given, [(name, seq)])] -> dict(stdout, contigs, parents_line, distinct);
    contigs is the -c table of the LAST assembly (the option takes one).  known = ((positions, distinct), rows) of expected(), for a single
    assembly whose counts the restatement has given already: only the text is made here"""
    batches = [(PAT, [s for _, s in f]) for f in pat_files] + [(MAT, [s for _, s in f]) for f in mat_files]
    if known:
        return cli_text(pat_files + mat_files, known[0][0], known[0][1], [(asm_files[0][0], asm_files[0][1], known[1])], k)
    P, M, n_pos = parent_sets(batches, k)
    return cli_text(pat_files + mat_files, n_pos, len(P | M), [(path, rs, phase(P, M, [s for _, s in rs], k)) for path, rs in asm_files], k)


def cli_text(parent_files, n_pos, distinct, asm_rows, k):
    """asm_rows: [(path, records, rows of phase())]"""
    recs = [r for f in parent_files for r in f]
    out = ["#file\tcontigs\tbases\tkmers\tpat\tmat\tpairs\tswitches\tswitch_rate\thamming\thamming_rate\n"]
    ctab = ""
    for path, rs, rows in asm_rows:
        kmers, pat, mat, pairs, sw, ham = totals(rows)
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (path, len(rs), sum(len(s) for _, s in rs), kmers, pat, mat, pairs, sw, rate(sw, pairs), ham,
                                                                   rate(ham, pat + mat)))
        ctab = "#contig\tlength\tkmers\tpat\tmat\tpp\tpm\tmp\tmm\n" + "".join("%s\t%d\t%s\n" % (n, len(s), "\t".join(map(str, r))) for (n, s), r in zip(rs, rows))
    line = "[trioeval] parents: %d records, %d bases, %d k-mers, %d distinct, k=%d" % (len(recs), sum(len(s) for _, s in recs), n_pos, distinct, k)
    return dict(stdout="".join(out).encode(), contigs=ctab.encode(), parents_line=line.encode(), distinct=distinct)


# ---- the constructions ----------------------------------------------------------------------------------------------------------------------------
def plant(rng, k, L, marks, filler=()):
    """a random contig of L bases and the k-mers at marks = [(position, type)] -> (contig, pat k-mers, mat k-mers).  filler = [(start, end)]: those
    stretches are random over the letters A and C only, so that no k-mer over all four letters recurs in them on either strand"""
    s = bytearray(kc.dna(rng, L))
    for a, b in filler:
        s[a:b] = bytes(rng.choices(b"AC", k=b - a))
    s = bytes(s)
    return s, [s[p:p + k] for p, t in marks if t == PAT], [s[p:p + k] for p, t in marks if t == MAT]


def planted(k, specs, seed):
    """specs: [(L, marks, filler)] per assembly contig -> (batches, query); every contig's markers are exactly its marks"""
    for attempt in range(200):
        rng = random.Random(seed * 1000 + 7 * k + attempt)
        q, pat, mat = [], [], []
        for L, marks, filler in specs:
            s, p, m = plant(rng, k, L, marks, filler)
            q.append(s)
            pat += p
            mat += m
        batches = [(PAT, pat), (MAT, mat)]
        P, M, _ = parent_sets(batches, k)
        if all(markers(P, M, s, k)[1] == sorted(marks) for s, (L, marks, _) in zip(q, specs)):
            return batches, q
    raise AssertionError("no seed gives the stated markers")


def mosaic(rng, k, L, n_het, n_switch, n_invalid=0):
    """-> (pat, mat, assembly): B with n_het substitutions in either parent, the assembly from alternating parents, cut at n_switch random offsets"""
    B = kc.dna(rng, L)
    offs = rng.sample(range(L), 2 * n_het)
    pat, mat = kc.sub(B, *offs[:n_het]), kc.sub(B, *offs[n_het:])
    cuts = [0] + sorted(rng.sample(range(1, L), n_switch)) + [L]
    asm = bytearray(b"".join((pat, mat)[i & 1][a:b] for i, (a, b) in enumerate(zip(cuts, cuts[1:]))))
    for o in rng.sample(range(L), n_invalid):
        asm[o] = ord("N")
    return pat, mat, bytes(asm)


@functools.lru_cache(maxsize=None)
def cases(k):
    """[(name, parental batches [(tag, [seq])], assembly [seq])]: every shape at which the kernels can go wrong, for one k"""
    rng = random.Random(2000 + k)
    out = []
    P_, M_ = PAT, MAT
    # markers at 63 and 64 (two words) and at TILE - 1 and TILE (two tiles), of equal and of different type: a switch exactly across each seam
    for name, a in (("word_seam", 63), ("tile_seam", TILE - 1)):
        L = a + 150
        specs = [(L, [(a, x), (a + 1, y)], ()) for x in (P_, M_) for y in (P_, M_)]
        specs += [(L, [(5, P_), (a, M_), (a + 1, M_), (a + 40, P_)], ()), (L, [(a - 1, M_), (a + 2, P_)], ()), (L, [(a + 1, M_)], ()), (L, [(a, P_)], ())]
        out.append((name,) + planted(k, specs, 1))
    # the only marker at L - k; contigs of 0, k - 1 and k bases (the last one a marker by itself)
    specs = [(TILE + 5 + k, [(TILE + 5, M_)], ()), (TILE + k - 1, [(TILE - 1, P_)], ()), (TILE + k, [(TILE, P_)], ()), (k, [(0, M_)], ()), (k - 1, [], ()), (0, [], ()), (k, [], ())]
    out.append(("last_position_and_short_contigs",) + planted(k, specs, 2))
    # a contig without markers between two with markers: no pair leaks across it, nor from one contig into the next
    specs = [(300, [(10, P_), (290 - k, P_)], ()), (TILE + 100, [], ()), (300, [(0, M_), (200, P_)], ()), (300, [(7, M_)], ()), (0, [], ()), (300, [(9, P_)], ())]
    out.append(("no_pair_across_contigs",) + planted(k, specs, 3))
    # a first tile and a last tile without a marker; markers only in the middle tile of three
    L = 3 * TILE
    specs = [(L, [(TILE + 3, P_), (2 * TILE + 900, M_)], ()), (L, [(77, M_), (2 * TILE - 1, M_)], ()), (L, [(TILE + 100, P_), (TILE + 101, M_), (2 * TILE - k, P_)], ()),
             (L, [(TILE - 1, P_), (2 * TILE, M_)], ())]
    out.append(("empty_first_and_last_tiles",) + planted(k, specs, 4))
    # more than 64 marker-free tiles between two markers: the seam walk takes a second round — in the first contig, and behind other contigs,
    # where the walk's lower bound is not tile 0; a contig whose first marker stands 66 tiles in: its walk ends at its own first tile, with no pair
    gap = 66 * TILE
    fill = [(TILE, gap)]
    specs = [(gap + TILE, [(100, P_), (gap + 5, M_)], fill), (500, [(400, M_)], ()), (gap + TILE, [(TILE - k, M_), (gap, M_), (gap + 64, P_)], fill),
             (gap + 2 * TILE, [(gap + 9, P_), (gap + TILE + 9, P_)], [(0, gap)])]
    out.append(("long_marker_free_stretches",) + planted(k, specs, 5))
    # a k-mer in both parents (tag 3) and one in neither between two markers; a parent that holds a marker's k-mer only as its reverse complement
    s = kc.dna(rng, 400)
    both, rc_only = s[100:100 + k], kc.revcomp(s[200:200 + k])
    batches = [(PAT, [s[50:50 + k], both, rc_only]), (MAT, [both, s[300:300 + k], kc.revcomp(s[320:320 + k])])]
    out.append(("both_neither_and_reverse_complement", batches, [s, kc.revcomp(s), s.lower()]))
    # an invalid byte between two markers: the pair still counts
    s = kc.dna(rng, 600)
    s = kc.put(kc.put(s, 150, ord("N")), 151 + k + 20, ord("-"))
    batches = [(PAT, [s[100:100 + k], s[500:500 + k]]), (MAT, [s[151:151 + k], s[300:300 + k]])]
    out.append(("invalid_between_markers", batches, [s, s[:155 + k] + b"N" * 100 + s[255 + k:]]))
    # homopolymer parents: every lane hits one slot, every position is a marker; a dense switch from A...A to C...C
    batches = [(PAT, [b"A" * (3 * TILE)]), (MAT, [b"C" * 100, b"g" * 50])]
    out.append(("homopolymer", batches, [b"A" * (2 * TILE + 100), b"T" * 100, b"a" * (TILE - 5) + b"C" * TILE, b"C" * (TILE + k) + b"T" * 70 + b"N" + b"G" * 64]))
    # the same key arrives first as pat and later as mat, and the other way round, in batches of their own
    x, y, z, w = (kc.dna(rng, 300) for _ in range(4))
    batches = [(PAT, [x]), (MAT, [z]), (MAT, [x, y]), (PAT, [z, w]), (PAT, [x[:100]]), (MAT, [z[100:]])]
    out.append(("tags_arrive_in_either_order", batches, [x + y, y + w, z, w + x, kc.revcomp(w) + y]))
    # every position of 1.2 tiles pat, mat, both or neither at random: dense words of every pattern
    s = kc.dna(rng, TILE + 800)
    kinds = rng.choices((0, PAT, MAT, 3), weights=(3, 3, 3, 1), k=len(s) - k + 1)
    batches = [(PAT, [s[i:i + k] for i, t in enumerate(kinds) if t & PAT]), (MAT, [s[i:i + k] for i, t in enumerate(kinds) if t & MAT])]
    out.append(("dense_random", batches, [s, s[5:TILE + 70]]))
    # the mosaic of the two parents: runs of k markers at every heterozygous site, switches at the cuts, a few invalid bytes
    pat, mat, asm = mosaic(rng, k, 3 * TILE + 123, 60, 7, 5)
    pat2, mat2, asm2 = mosaic(rng, k, TILE + 1, 30, 3)
    out.append(("mosaic", [(PAT, [pat, pat2[:600]]), (MAT, [mat]), (PAT, [pat2[600 - k + 1:]]), (MAT, [mat2])], [asm, asm2, pat, mat2, asm[TILE - 50:2 * TILE + 50]]))
    return out


FULL_TABLE_CASES = ("mosaic", "dense_random", "homopolymer", "tags_arrive_in_either_order", "word_seam")


@functools.lru_cache(maxsize=None)
def expected(k):
    """{name: (batches, query, (positions, distinct), rows)}: computed once per k and shared"""
    out = {}
    for name, batches, query in cases(k):
        P, M, n_pos = parent_sets(batches, k)
        out[name] = (batches, query, (n_pos, len(P | M)), phase(P, M, query, k))
    return out
