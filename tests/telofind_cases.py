"""Shared by tests/test_gpu_telofind_seams.py and tests/test_telofind_cases_host.py: inputs that put tf_scan (cornetto_amd/csrc/telo.hip) on
its own seams, and what the oracle says about them.  Generators and the oracle only: no device code here.

tf_scan gives each of 254 threads 64 positions of a tile (threads 0 and 255 hold the neighbouring tiles' last and first 64), a workgroup takes
four consecutive tiles and refills its registers with the next tile's bytes while it computes, and a tile's run heads and tails go into fixed
rows of 32.  So a copy of the motif can be cut by a segment seam (two threads of one tile), by a tile seam inside a workgroup (the halo
threads, the refilled registers) or by a tile seam between two workgroups (a "group" seam: global tile index a multiple of 4).  seam_case()
plants copies at every split over each kind, row_case() fills one tile's lists to exactly 32 and 33 entries, dense_case() to the most a tile
can hold.  expected() returns the oracle's hit rows, the mark words built from them and `car` of every window (thr_adj = 0); census() says
from the layout which splits over which seam kind a case really holds, so that tests/test_telofind_cases_host.py can refuse a generator
that lost one."""
import zlib

import numpy as np

import cornetto_amd
import oracle_bind as ob

HIT, WIN = cornetto_amd.HIT_DT, cornetto_amd.WIN_DT

SEG = 64                   # telo.hip: TF_SEG, positions per thread
TILE = 16256               # telo.hip: TF_TILE = (TF_THREADS - 2) * TF_SEG
NT = 4                     # telo.hip: TF_NT, consecutive tiles per workgroup
ROW = 32                   # telo.hip: TF_ROW, list entries of a tile in single-pass mode
MAX_MOTIF = 32             # telo.hip: MAX_MOTIF, the longest motif of the 32-bit automaton

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = b"ACGT"


def revcomp(m):
    return m.translate(_COMP)[::-1]


def border(m):
    """has_border() of telo.hip: a proper prefix of m that is also its suffix"""
    return any(m[:b] == m[-b:] for b in range(1, len(m)))


def period(m):
    """the shortest p with m[i] == m[i - p] throughout (len(m) for a motif without a border)"""
    return next(p for p in range(1, len(m) + 1) if all(m[i] == m[i - p] for i in range(p, len(m))))


def template(m):
    """the instantiation of tf_scan that telofind_impl picks: H = 7, 15, 31, or -1 (byte-wise) beyond MAX_MOTIF"""
    k = len(m)
    return -1 if k > MAX_MOTIF else 7 if k <= 8 else 15 if k <= 16 else 31


# ---- the motifs -------------------------------------------------------------------------------------------------------------------------------
UNBORDERED = (
    b"G",                                      # k = 1: smear() without a loop step, no split possible, heads = tails
    b"AC",                                     # k = 2: the shortest motif a seam can cut
    b"ACG",                                    # ACG / CGT: the marks of the two strands overlap where ACGT stands
    b"ACGT",                                   # its own reverse complement: both strands report every run
    b"TTAGGG",                                 # the vertebrate unit, the product's default
    b"CCCTAA",                                 # the same with the strands' roles exchanged
    b"TTTAGGG",                                # the plant unit: k = 7, one wildcard position left in H = 7
    b"CAGATTTT",                               # k = 8: H = 7 with no wildcard, INJ2 on the lowest bits of both automata
    b"CATATTATG",                              # k = 9: the shortest motif of H = 15
    b"CAGAAAATCTACTTCG",                       # k = 16: H = 15 with no wildcard
    b"CCTGATACGAGTCGGTT",                      # k = 17: the shortest motif of H = 31
    b"ATCTTCGGATACTGTATAGTCCCACCTGGTG",        # k = 31: one wildcard position in H = 31
    b"ATCCTATGCTTGTGAGTACCCAGAAAATAGCG",       # k = 32 = MAX_MOTIF: H = 31 with no wildcard, INJ = bit 0
)
BORDERED = (                                   # k <= 32 with a border: every match listed, runs by tf_greedy
    b"AAAA",                                   # period 1: a match at every position of a stretch
    b"ACAC",                                   # period 2, k a multiple of it
    b"ACACA",                                  # period 2, k not a multiple of it: the greedy rule skips off-phase matches
    b"TTAGGGTT",                               # period 6 under k = 8 < 2 p: H = 7 without a wildcard, bordered
    b"ACGT" * 8,                               # k = 32, period 4, its own reverse complement
)
LONG = (                                       # k > 32: tf_scan<-1> compares byte by byte
    b"G" * 33,                                 # the first length beyond the automaton, period 1
    b"TTAGGG" * 6,                             # 36: six units
    b"GGGTTA" * 11 + b"G",                     # 67: longer than a segment
    b"TATACATAGAACGTGTTAGGGCAGAATTAGCGGTAAACTCAACGAGGTAGCAAGGCCACGACTTGCCCAG",          # 70, no border
    b"GGACAAGTGCGGCCTTAAGCGCGCGTGCGTAACTGGGATTATAAACACCACCCTGTTCGGAGGAGCCCGGTGCTGACGACTCGGGTGCGAACTAGCTGGTG"
    b"AGGCTCATATATCGACATGCTTTTGCGTAAAGTCGTCCGATTGGCATTTGTTGGGCATTCTGGGATTGTTGTCTTACCGTAGCGGGATGTTGTTGAACC",       # 200, no border: spans four segments
)
MOTIFS = UNBORDERED + BORDERED + LONG

for _m in UNBORDERED:
    assert len(_m) <= MAX_MOTIF and not border(_m) and not border(revcomp(_m)), _m
    assert (_m == revcomp(_m)) == (_m == b"ACGT"), _m
assert sorted(len(m) for m in UNBORDERED) == [1, 2, 3, 4, 6, 6, 7, 8, 9, 16, 17, 31, 32]
assert {template(m) for m in UNBORDERED} == {7, 15, 31}
for _m in BORDERED:
    assert len(_m) <= MAX_MOTIF and border(_m) and border(revcomp(_m)) and period(_m) < len(_m), _m
assert [period(m) for m in BORDERED] == [1, 2, 2, 6, 4] and BORDERED[4] == revcomp(BORDERED[4])
for _m in LONG:
    assert len(_m) > MAX_MOTIF and template(_m) == -1, _m
assert [len(m) for m in LONG] == [33, 36, 67, 70, 200] and [border(m) for m in LONG] == [True, True, True, False, False]
assert len(set(MOTIFS)) == len(MOTIFS)


# ---- the reference's rule on a short text (src/find_telomere.c:49-58), in Python: what a plant holds on its own --------------------------------
def runs_of(text, pat):
    """[(start, end)]: the next occurrence at or after pos, extended while the next k bytes are the pattern, resumed one behind the end"""
    k, pos, out = len(pat), 0, []
    while True:
        i = text.find(pat, pos)
        if i < 0:
            return out
        e = i
        while text[e:e + k] == pat:
            e += k
        out.append((i, e))
        pos = e + 1


def occurrences(text, pat):
    """every start of pat in text, overlapping ones included"""
    out, i = [], text.find(pat)
    while i >= 0:
        out.append(i)
        i = text.find(pat, i + 1)
    return out


# ---- seam_case ----------------------------------------------------------------------------------------------------------------------------------
CTG_LEN = 4 * TILE + 200                       # 5 tiles: consecutive contigs put the group seam on each in-contig tile seam in turn
TILE_SEAMS = (TILE, 2 * TILE, 3 * TILE, 4 * TILE)
SEG_SEAMS = (64, TILE - 64, TILE + 64, 4 * TILE + 64, 128, 256)
GAP = 2                                        # bases of filler between two plants at the least: each has flanking letters of its own
LONG_D = (0, 1, 31, 32, 33, 63, 64, 65)        # k > 32: these, k - 1 and k


def filler_letters(motif):
    """the two letters that are neither x nor its complement, x the first of A, T, G, C that the motif holds: the motif and its reverse
    complement then occur only where a plant brings an x (or its complement) along"""
    x = next(c for c in b"ATGC" if c in motif)
    return bytes(c for c in ACGT if c not in (x, _COMP[x]))


def split_list(motif):
    """the splits d a case is built for: a plant starts d letters in front of the seam"""
    k = len(motif)
    if k <= MAX_MOTIF:
        return list(range(k + 1))
    return sorted(d for d in set(LONG_D + (k - 1, k)) if d <= k)


def stretch_lengths(motif):
    k, p = len(motif), period(motif)
    return sorted({k, k + 1, k + p, 2 * k - 1, 2 * k, 2 * k + 1, 3 * k})


def stretch_splits(motif, L):
    """k <= 8: every start of the stretch in front of the seam.  Longer motifs: 0 .. p and k - p .. k + 1 (the occurrences inside a stretch stand
    at multiples of p, so these starts put every split 1 .. k - 1 of an occurrence on the seam), L - 1 and L"""
    k, p = len(motif), period(motif)
    if k <= 8:
        return list(range(L + 1))
    return sorted(d for d in set(range(0, p + 1)) | set(range(k - p, k + 2)) | {L - 1, L} if 0 <= d <= L)


def overlap_text(motif):
    """the shortest text in which the motif and its reverse complement overlap (ACG: ACGT, marked by both strands), or None"""
    rc, k = revcomp(motif), len(motif)
    return next((motif + rc[k - o:] for o in range(1, k) if motif[o:] == rc[:k - o]), None) if motif != rc else None


def uses_stretches(motif):
    return len(motif) <= MAX_MOTIF and (border(motif) or border(revcomp(motif)))


def _specs(motif):
    """one contig each: (text to plant, its period, the unit, d, priority of the segment seams over the contig ends)"""
    rc = revcomp(motif)
    units = (motif,) if motif == rc else (motif, rc)
    out = []
    if uses_stretches(motif):
        p = period(motif)
        for li, L in enumerate(stretch_lengths(motif)):
            for di, d in enumerate(stretch_splits(motif, L)):
                for ui, u in enumerate(units):
                    out.append(((u[:p] * (L // p + 1))[:L], p, u, d, (li + di + ui) % 2 == 0))
    else:
        for di, d in enumerate(split_list(motif)):
            for ci, c in enumerate((1, 2, 3)):
                for ui, u in enumerate(units):
                    out.append((u * c, len(u), u, d, (di + ci + ui) % 2 == 0))
    return out


def n_contigs(motif):
    """the contigs of seam_case(motif)"""
    return len(_specs(motif))


def decoy_seams(ci):
    """every fifth contig gives two of its tile seams to decoys instead of copies: (seam of the unit with its last letter replaced, seam of
    the unit with its first letter replaced) as multiples of TILE, one of them the contig's group seam; None for the other contigs"""
    if ci % 5 != 4:
        return None
    jg = (-5 * ci) % NT or NT                  # first tile 5 ci: tile 5 ci + jg opens a workgroup
    jt = jg % 4 + 1
    return (jg, jt) if ci // 5 % 2 == 0 else (jt, jg)


class Case:
    """seqs: uint8 arrays; plants: per contig [(position, upper-case text, kind)], kind "copy" (copies or a stretch) or "decoy"; first_tile: the
    global index of every contig's first tile (and the number of tiles behind the last)"""

    def __init__(self, motif, seqs, plants):
        self.motif, self.seqs, self.plants = motif, seqs, plants
        self.first_tile = np.concatenate([[0], np.cumsum([-(-len(s) // TILE) for s in seqs])]).astype(np.int64)


def _place(taken, pos, n, length):
    """True, and the interval noted, when [pos, pos + length) lies in the contig at least GAP away from every plant so far"""
    if pos < 0 or pos + length > n or any(pos < b + GAP and a < pos + length + GAP for a, b in taken):
        return False
    taken.append((pos, pos + length))
    return True


def seam_case(motif):
    """see the module text and the issue: every split d of a copy (of a stretch, for a motif with a border) over every seam, 1 to 3 copies,
    both units, decoys that differ in their first or last letter, lower case in half of the contigs.

    Plants are placed in order of priority and one that does not fit is dropped (_place): first the tile seams, which always fit except
    4 TILE under three long copies; then the segment seams and the two contig ends, in an order that alternates between contigs (a long
    plant at 64 - d leaves no room for one at 128 - d or at 0); then the overlap text, then the decoys.  What holds in spite of that is
    checked by tests/test_telofind_cases_host.py: census() has every split over every kind of seam, both strands have a run at a contig's
    first base and one at its last, every contig has a decoy.
    Decoys: in every contig the unit with its first letter replaced lies over a SEGMENT seam behind tile seam jd and the unit with its last
    letter replaced over one in front of it (the tile seam itself belongs to the copy); in every fifth contig two TILE seams, one of them
    the group seam, carry such decoys instead of copies (decoy_seams), so that a unit one letter off also crosses the halo threads and the
    refilled registers."""
    k = len(motif)
    fill = np.frombuffer(filler_letters(motif), dtype=np.uint8)
    rng = np.random.default_rng([20261021, k, zlib.crc32(motif)])
    seqs, plants = [], []
    for ci, (text, per, unit, d, segs_first) in enumerate(_specs(motif)):
        n, L = CTG_LEN, len(text)
        s = fill[rng.integers(0, 2, size=n)].copy()
        taken, mine = [], []
        ends = (0, n - L)
        dd = min(max(d, 1), k - 1)
        first = bytes([next(c for c in fill if c != unit[0])]) + unit[1:]
        last = unit[:-1] + bytes([next(c for c in fill if c != unit[-1])])
        over = decoy_seams(ci) if k >= 2 else None
        if over:
            for j, dec in zip(over, (last, first)):
                if _place(taken, j * TILE - dd, n, k):
                    mine.append((j * TILE - dd, dec, "decoy"))
        spots = [S - d for S in TILE_SEAMS if not over or S // TILE not in over]
        spots += [S - d for S in SEG_SEAMS] + list(ends) if segs_first else list(ends) + [S - d for S in SEG_SEAMS]
        for pos in spots:
            if _place(taken, pos, n, L):
                mine.append((pos, text, "copy"))
                # the letters beside the plant do not continue it
                if pos > 0:
                    s[pos - 1] = next(c for c in fill if c != text[per - 1])
                if pos + L < n:
                    s[pos + L] = next(c for c in fill if c != text[L - per])
        both = overlap_text(motif)
        if both and _place(taken, 2 * TILE + 192 - d, n, len(both)):
            mine.append((2 * TILE + 192 - d, both, "copy"))
        if k >= 2:
            # decoys beside the tile seam jd, each cut by a segment seam: the unit with its first / its last letter replaced by filler
            # (far enough from the seam's own plant of up to three copies)
            jd, off = 1 + ci % 3, 128 if k <= 16 else SEG * ((4 * k + GAP) // SEG + 2)
            for S, dec in ((jd * TILE + off, first), (jd * TILE - off, last)):
                if _place(taken, S - dd, n, k):
                    mine.append((S - dd, dec, "decoy"))
        for pos, t, _ in mine:
            s[pos:pos + len(t)] = np.frombuffer(t, dtype=np.uint8)
        if ci % 4 in (1, 2):
            s[rng.random(n) < 0.3] |= 0x20
        seqs.append(s)
        plants.append(sorted(mine))
    return Case(motif, seqs, plants)


def planted(case):
    """the HIT rows the plants hold, each taken on its own, in print order (contig, strand, position)"""
    motif, rc = case.motif, revcomp(case.motif)
    rows = []
    for ci, pl in enumerate(case.plants):
        for strand, pat in enumerate((motif, rc)):
            rows += [(ci, strand, pos + a, pos + b) for pos, t, _ in pl for a, b in runs_of(t, pat)]
    return np.array(rows, dtype=HIT).reshape(-1)


def decoy_census(case):
    """{"segment" | "tile" | "group": the splits at which a decoy lies over a seam of that kind}"""
    out = {"segment": set(), "tile": set(), "group": set()}
    for ci, pl in enumerate(case.plants):
        for pos, t, kind in pl:
            if kind == "decoy":
                for m in range((pos // SEG + 1) * SEG, pos + len(t), SEG):
                    out[seam_kind(case, ci, m)].add(m - pos)
    return out


def decoy_spans(case):
    """[(contig, start, end)] of every decoy"""
    return [(ci, pos, pos + len(t)) for ci, pl in enumerate(case.plants) for pos, t, kind in pl if kind == "decoy"]


def seam_kind(case, ci, m):
    """position m of contig ci, a multiple of SEG inside the contig: "group" (a tile seam whose second tile opens a workgroup), "tile" or "segment" """
    if m % TILE:
        return "segment"
    return "group" if (int(case.first_tile[ci]) + m // TILE) % NT == 0 else "tile"


def census(case):
    """{"segment" | "tile" | "group": the splits d such that an occurrence of the motif or of its reverse complement in a plant has d letters in
    front of a seam of that kind and k - d behind it}, from the layout alone"""
    motif, rc = case.motif, revcomp(case.motif)
    k = len(motif)
    out = {"segment": set(), "tile": set(), "group": set()}
    for ci, pl in enumerate(case.plants):
        for pos, t, kind in pl:
            if kind != "copy":
                continue
            for o in sorted(set(occurrences(t, motif) + occurrences(t, rc))):
                q = pos + o
                for m in range((q // SEG + 1) * SEG, q + k, SEG):
                    out[seam_kind(case, ci, m)].add(m - q)
    return out


# ---- row_case -----------------------------------------------------------------------------------------------------------------------------------
ROW_MOTIF = b"TTAGGG"
ROW_CTG = 3 * TILE                             # three whole tiles
ROW_WHERE = ("mid", "first", "last", "flush", "tail_next", "head_prev")
ROW_STEP = 13                                  # isolated copies: 6 letters and 7 of filler


# (n_fwd, n_rev, where, the designated tile's [heads fwd, tails fwd, heads rev, tails rev]): 32 stays in the rows, 33 in any list overflows
ROW_CASES = [(32, 0, "mid", (32, 32, 0, 0)), (0, 32, "mid", (0, 0, 32, 32)), (32, 32, "mid", (32, 32, 32, 32)),
             (33, 0, "mid", (33, 33, 0, 0)), (0, 33, "mid", (0, 0, 33, 33)),
             (32, 0, "tail_next", (33, 32, 0, 0)), (32, 0, "head_prev", (32, 33, 0, 0)), (32, 0, "flush", (32, 32, 0, 0)),
             (32, 32, "first", (32, 32, 32, 32)), (33, 0, "first", (33, 33, 0, 0)), (32, 32, "last", (32, 32, 32, 32)), (0, 33, "last", (0, 0, 33, 33))]


def row_at(where):
    """(contig, tile) of the designated tile"""
    return {"first": (0, 0), "last": (2, 2)}.get(where, (1, 1))


def row_case(n_fwd, n_rev, where="mid"):
    """three contigs of three tiles; the designated tile holds n_fwd isolated copies of TTAGGG and n_rev of CCCTAA at least 7 bases apart, every
    other tile three of each.  where: "mid" (1, 1), "first" / "last" tile of the assembly; "flush": the last forward copy ends with the tile;
    "tail_next": one forward run more whose first copy begins in the tile and whose second begins in the next (a head here, its tail there);
    "head_prev": one forward run more whose first copy begins in the previous tile and whose second begins in this one (its tail here)"""
    assert where in ROW_WHERE
    fill = np.frombuffer(filler_letters(ROW_MOTIF), dtype=np.uint8)
    rng = np.random.default_rng([20261022, n_fwd, n_rev, ROW_WHERE.index(where)])
    at = row_at(where)
    seqs, plants = [], []
    for c in range(3):
        s = fill[rng.integers(0, 2, size=ROW_CTG)].copy()
        mine = []
        for tl in range(3):
            t0 = tl * TILE
            nf, nr = (n_fwd, n_rev) if (c, tl) == at else (3, 3)
            spots = [t0 + 100 + ROW_STEP * i for i in range(nf + nr)]
            if (c, tl) == at and where == "flush" and nf:
                spots[nf - 1] = t0 + TILE - 6
            for i, p in enumerate(spots):
                mine.append((p, ROW_MOTIF if i < nf else revcomp(ROW_MOTIF), "copy"))
            if (c, tl) == at and where == "tail_next":
                mine.append((t0 + TILE - 4, ROW_MOTIF * 2, "copy"))
            if (c, tl) == at and where == "head_prev":
                mine.append((t0 - 4, ROW_MOTIF * 2, "copy"))
        for p, t, _ in mine:
            s[p:p + len(t)] = np.frombuffer(t, dtype=np.uint8)
        seqs.append(s)
        plants.append(sorted(mine))
    return Case(ROW_MOTIF, seqs, plants)


def list_counts(case, rows):
    """{(contig, tile): [heads fwd, tails fwd, heads rev, tails rev]} of HIT rows: a head is a run's start, a tail its end - k"""
    k, out = len(case.motif), {}
    for r in rows:
        for q, p in ((2 * int(r["strand"]), int(r["start"])), (2 * int(r["strand"]) + 1, int(r["end"]) - k)):
            out.setdefault((int(r["ctg"]), p // TILE), [0, 0, 0, 0])[q] += 1
    return out


# ---- dense_case ---------------------------------------------------------------------------------------------------------------------------------
DENSE_LEN = 2 * TILE + 3


def dense_case():
    """[(seqs, motif)]: GC alternating under motif G — heads and tails of both strands at every other position, 8128 entries in each of the
    four lists of a full tile, the most a motif without a border can give; poly-A and poly-T under AAAA — a match at every position, 16256
    entries in list 0 (the first contig) and in list 2 (the second)"""
    gc = np.frombuffer(b"GC" * (DENSE_LEN // 2 + 1), dtype=np.uint8)[:DENSE_LEN].copy()
    return [([gc], b"G"), ([np.full(DENSE_LEN, ord("A"), np.uint8), np.full(DENSE_LEN, ord("T"), np.uint8)], b"AAAA")]


def match_counts(seqs, motif):
    """{(contig, tile): [matches fwd, matches rev]}: every occurrence, overlapping ones included, binned by its start"""
    out = {}
    for ci, s in enumerate(seqs):
        text = bytes(s).upper()
        for q, pat in enumerate((motif, revcomp(motif))):
            for p in occurrences(text, pat):
                out.setdefault((ci, p // TILE), [0, 0])[q] += 1
    return out


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------------
def n_words(seqs):
    return sum(-(-len(s) // 64) for s in seqs)


def expected(seqs, motif):
    """(HIT rows in print order, the mark words, WIN rows at thr_adj = 0).  Rows: oracle_bind.telofind per contig.  Words: the union of
    [start, end) over the runs of both strands, every contig from a multiple of 64 bits, little-endian in uint64, the bits behind a contig's
    end zero.  Windows: oracle_bind.telowin over the same runs at threshold 0, `car` of every window the reference visits."""
    rows, words, wins = [], [], []
    for ci, s in enumerate(seqs):
        oh = ob.telofind(s, motif)
        r = np.zeros(len(oh), dtype=HIT)
        r["ctg"], r["strand"], r["start"], r["end"] = ci, oh["strand"], oh["start"], oh["end"]
        rows.append(r)
        bits = np.zeros(-(-len(s) // 64) * 64, dtype=np.uint8)
        for a, b in zip(oh["start"], oh["end"]):
            bits[int(a):int(b)] = 1
        words.append(np.packbits(bits, bitorder="little").view("<u8"))
        ow = ob.telowin(oh, len(s), 0.0)
        w = np.zeros(len(ow), dtype=WIN)
        w["ctg"], w["start"], w["end"], w["car"] = ci, ow["start"], ow["end"], ow["car"]
        wins.append(w)
    return (np.concatenate(rows) if rows else np.zeros(0, HIT), np.concatenate(words).astype(np.uint64) if words else np.zeros(0, np.uint64),
            np.concatenate(wins) if wins else np.zeros(0, WIN))
