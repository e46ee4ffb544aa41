"""Shared by tests/test_gpu_telowin.py, the hit-list goldens (tests/golden/make_golden_telowin_hits.py) and the host CLI test: explicit hit
lists for `telowin` that telofind never writes — overlapping, repeated, unsorted, one base long, inside one 64-bit word, ending or starting
on a word boundary, empty — on contig lengths at every seam of the window rule (src/telomere_windows.c:31-41) and of its device form
(csrc/telowin_tile.hpp: words of 64 marks, blocks of 200, tiles of 256 windows = 51 200 bases), marks that put car / den exactly on the
threshold, and thousands of one-window contigs for the copy-back of the result.  Generators and the oracle only: no device code here.

A case is {"lens": int32 lengths, "hits": HIT rows (ctg, strand, start, end) in file order, "names": contig names}.  With thr_adj = 0
every window the reference's loop visits passes (0 / 0 on an empty contig is NaN and does not), so the expectation holds `car` of EVERY
window and the visiting rule itself."""
import functools

import numpy as np

import cornetto_amd
import oracle_bind as ob

HIT, WIN = cornetto_amd.HIT_DT, cornetto_amd.WIN_DT
cached = functools.lru_cache(maxsize=None)

# 52 000 is the last length with one window tile (J = 255), 52 001 the first with two (window 256 alone in the second); 103 2xx crosses
# into a third.  1000 / 1001 and 1200 / 1201: the first lengths with a second and a third window.
SEAM_LENS = (0, 1, 63, 64, 65, 199, 200, 201, 999, 1000, 1001, 1199, 1200, 1201, 1400, 2000, 51999, 52000, 52001, 52199, 52200, 52201, 103200, 103201,
             103401)
HIT_LENS = (1, 2, 63, 64, 65, 128, 200, 777, 1000, 1300)
FILL_BLOCK = 256           # telo.hip: hits per workgroup of tw_fill


def n_windows(n):
    """the windows the loop of src/telomere_windows.c:31-41 visits and, at thr_adj = 0, prints: i = 0, 200, ... up to and including the first
    i with i + 1000 >= n; den = 0 on an empty contig prints nothing"""
    if n == 0:
        return 0
    return 1 + (-(-(n - 1000) // 200) if n > 1000 else 0)


def _case(lens, per_ctg, names=None):
    rows = [(c, st, a, b) for c, hs in enumerate(per_ctg) for a, b, st in hs]
    return {"lens": np.array(lens, np.int32), "hits": np.array(rows, dtype=HIT).reshape(-1),
            "names": names or [b"s%d" % n for n in lens]}


def _seam_hits(rng, n, n_random, whole):
    """[(start, end, strand)] of one contig of length n > 0, shuffled"""
    hs = []
    # anchors a hit may start or end at: word, block and tile seams, the last windows
    anchors = [a for a in (64, 128, 192, 200, 400, 1000, 1024, 51200, 51264, 52000, 102400, n - 1000, n - 1200, n - 64, n) if 0 < a <= n]
    for k in range(n_random):
        ln = HIT_LENS[int(rng.integers(0, len(HIT_LENS)))]
        if k % 2 and anchors:                                   # ends on / starts on / straddles a seam
            a = anchors[int(rng.integers(0, len(anchors)))]
            s = a - (0, ln, ln // 2, 1)[int(rng.integers(0, 4))]
        else:
            s = int(rng.integers(0, n))
        s = min(max(0, s), n - 1)
        hs.append((s, min(n, s + ln), int(rng.integers(0, 2))))
    hs += [hs[int(rng.integers(0, len(hs)))] for _ in range(3)]  # exact duplicates
    hs += [(p, p + 1, int(rng.integers(0, 2))) for p in (0, 63, 64, 127, 128, n - 1) if p < n]
    if n >= 128:
        hs.append((64, 128, 0))                                 # one whole word: lo == 0 and hi == 64
    if whole:
        hs.append((0, n, 1))
    p = int(rng.integers(0, n + 1))
    hs.append((p, p, 0))                                        # start == end and start > end: the reference's marking loop does nothing
    hs.append((n, max(0, n - 70), 1))
    return [hs[i] for i in rng.permutation(len(hs))]


@cached
def seam_contigs(whole=False):
    """the table of SEAM_LENS.  whole=False: about 40 random hits per contig and more than two workgroups of tw_fill; whole=True: the
    second variant, every contig also covered by one hit from end to end (car = den in every window whatever else is marked) under
    fewer random hits — more than one workgroup of tw_fill, fewer than three.  One name comes back later in the table: a new contig, as
    in the reference (src/telomere_windows.c:69)."""
    rng = np.random.default_rng(20261020 + whole)
    per = [_seam_hits(rng, n, 8 if whole else 40, whole) if n else [(0, 0, 0)] for n in SEAM_LENS]
    names = [b"s%d" % n for n in SEAM_LENS]
    names[SEAM_LENS.index(1400)] = names[SEAM_LENS.index(200)]
    case = _case(SEAM_LENS, per, names)
    marking = int((case["hits"]["start"] < case["hits"]["end"]).sum())
    assert (FILL_BLOCK < marking <= 2 * FILL_BLOCK) if whole else marking > 2 * FILL_BLOCK, marking
    return case


def variants(case):
    """the same marks written another way: the hits of each contig sorted by start, and every hit given twice"""
    h = case["hits"]
    srt = h[np.lexsort((h["end"], h["start"], h["ctg"]))]
    twice = np.repeat(h, 2)
    return {"sorted": dict(case, hits=srt), "twice": dict(case, hits=twice)}


def tsv(case):
    """the six columns of `telofind` (src/find_telomere.c:51): name, length, strand, start, end, end - start"""
    names, lens = case["names"], case["lens"]
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (names[h["ctg"]], lens[h["ctg"]], h["strand"], h["start"], h["end"], h["end"] - h["start"])
                    for h in case["hits"])


def stderr_line(identity, thr):
    """what `telowin <file> identity thr` says on stderr before it reads the file (src/telomere_windows.c:53-55)"""
    ident = float(identity) / 100
    return b"Given error rate of %.6f running with adjusted threshold of %.6f due to survival prob %.6f\n" % (
        ident, ob.telowin_threshold(float(thr), float(identity)), pow(ident, 6))


def expected(case, thr):
    """the oracle's rows (ctg, start, end, car), contig by contig (oracle_bind.telowin is pinned to the reference: tests/test_oracle_golden.py)"""
    h, lens = case["hits"], case["lens"]
    order = np.argsort(h["ctg"], kind="stable")
    h = h[order]
    cut = np.searchsorted(h["ctg"], np.arange(len(lens) + 1))
    oh = np.zeros(len(h), dtype=ob.HIT_DT)
    oh["start"], oh["end"], oh["strand"] = h["start"], h["end"], h["strand"]
    parts = []
    for c, n in enumerate(lens):
        w = ob.telowin(oh[cut[c]:cut[c + 1]], int(n), thr)
        if thr == 0:
            assert len(w) == n_windows(int(n)), (int(n), len(w))
        out = np.zeros(len(w), dtype=WIN)
        out["ctg"], out["start"], out["end"], out["car"] = c, w["start"], w["end"], w["car"]
        parts.append(out)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=WIN)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
TIE = (0.5, 100.0)         # identity 100: the adjusted threshold is the threshold itself, and 0.5 is a double


@cached
def tie_contigs():
    """car / den exactly on the threshold and one mark beside it (`>=` at src/telomere_windows.c:37):
    contig 0: window [0, 1000) holds 500 marks and passes, its neighbour [200, 1200) holds 499 and does not;
    contig 1 (600 bases): the one clipped window has den = 600, car = 300 and passes;
    contig 2 (601 bases): den = 601, car = 300 and does not.
    The marks come in overlapping pieces."""
    thr = ob.telowin_threshold(*TIE)
    assert thr == 0.5
    case = _case([3000, 600, 601], [[(250, 500, 0), (0, 300, 1), (1000, 1199, 0), (1100, 1150, 1)],
                                    [(100, 300, 0), (0, 200, 0)],
                                    [(301, 450, 1), (440, 601, 0), (600, 601, 1)]])
    every = {(int(w["ctg"]), int(w["start"])): (int(w["end"]), int(w["car"])) for w in expected(case, 0.0)}
    assert every[(0, 0)] == (1000, 500) and every[(0, 200)] == (1200, 499) and every[(1, 0)] == (600, 300) and every[(2, 0)] == (601, 300)
    passing = {(int(w["ctg"]), int(w["start"])) for w in expected(case, thr)}
    assert (0, 0) in passing and (0, 200) not in passing and (1, 0) in passing and (2, 0) not in passing, passing
    return case


# ---- many windows -------------------------------------------------------------------------------------------------------------------------
@cached
def many_windows(n_ctg):
    """n_ctg contigs of 1 to 3 bases, every third one marked with a 1-base hit: at thr_adj = 0 exactly n_ctg windows, one workgroup of
    tw_scan each"""
    lens = 1 + np.arange(n_ctg, dtype=np.int32) % 3
    ctg = np.arange(0, n_ctg, 3, dtype=np.int32)
    hits = np.zeros(len(ctg), dtype=HIT)
    hits["ctg"], hits["strand"] = ctg, ctg & 1
    hits["start"] = lens[ctg] - 1
    hits["end"] = lens[ctg]
    return {"lens": lens, "hits": hits, "names": None}


# ---- the same seams through the telofind pass -----------------------------------------------------------------------------------------------
MOTIF = b"TTAGGG"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@cached
def seam_assembly():
    """contigs of SEAM_LENS of random bases with runs of TTAGGG / CCCTAA planted so that they end on, start on and straddle positions 64 k,
    200 k and 51 200 (the first base of the second window tile) -> list of uint8 arrays"""
    rng = np.random.default_rng(20261021)
    seqs = []
    for n in SEAM_LENS:
        s = ACGT[rng.integers(0, 4, size=n)].copy()
        seams = [p for p in (64, 128, 200, 400, 960, 1000, 1024, 1200, 51200, 51264, 51400, 52000, 102400, 102464, n - 1000, n) if 0 < p <= n]
        seams += [int(x) * 64 for x in rng.integers(1, max(2, n // 64), size=6) if int(x) * 64 <= n]
        seams += [int(x) * 200 for x in rng.integers(1, max(2, n // 200), size=6) if int(x) * 200 <= n]
        for i, p in enumerate(seams):
            unit = (MOTIF, b"CCCTAA")[i % 2]
            k = 6 * int(rng.integers(1, 60))
            a = (p - k, p, p - k // 2 - int(rng.integers(0, 6)))[i % 3]     # ends on the seam / starts on it / straddles it
            a = max(0, a)
            rep = np.frombuffer(unit * (k // 6), dtype=np.uint8)[:n - a]
            s[a:a + len(rep)] = rep
        seqs.append(s)
    return seqs


def expected_scan(seqs, thr, motif=MOTIF):
    """(HIT rows, WIN rows) of ob.telofind + ob.telowin over the records"""
    hits, wins = [], []
    for ci, s in enumerate(seqs):
        oh = ob.telofind(s, motif)
        hits += [(ci, int(h["strand"]), int(h["start"]), int(h["end"])) for h in oh]
        ws = ob.telowin(oh, len(s), thr)
        if thr == 0:
            assert len(ws) == n_windows(len(s))
        wins += [(ci, int(w["start"]), int(w["end"]), int(w["car"])) for w in ws]
    return np.array(hits, dtype=HIT).reshape(-1), np.array(wins, dtype=WIN).reshape(-1)
