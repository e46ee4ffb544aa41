"""Planted inputs for sd_sift (cornetto_amd/csrc/sdust_sift.hpp), the sdust kernel of W <= 66 and 5 <= T <= 100000 — CPU only, no device.
tests/test_sift_cases_host.py checks the cases themselves, tests/test_gpu_sdust_sift.py runs them on the device against the oracle's intervals
kept here.  The pattern is that of _case() / _check_planted() in tests/test_gpu_sdust_wide.py (whose small helpers live here now).

case(T, W, cvals) builds ONE assembly planted for every chunk size of cvals and keeps the oracle's intervals with it (computed once, cached).
check(k) asserts that every kind below is present for every chunk size and that the oracle reports an interval over every planted repeat, so
an emptied case fails instead of passing; for the pairs of EMPTY no interval can exist and the oracle's list must be empty.

At the borders B = k c of every chunk size c (one border per kind and size, a neighbourhood of its own):
  a     a repeat that straddles B                      b1 / b2   one that ends / starts exactly at B
  f     two repeats closer than W, B in the gap        g         two homopolymers of different letters end to end, B between the times the
  case  as a, the neighbourhood in lower case                    two are recorded: only the stitch can merge them
  r0 r1 r2   a repeat that starts exactly at B - W - 1, B - W, B - W + 1 (a clean chunk records the starts in [start - W, end - W))
  t32 t64    a repeat that straddles B + 32 / B + 64: the half-wave border of the equal-word tables and a tile border
  s / s2     (c >= 1024) a repeat that straddles region offset 1024 = B + 896, where lane 0 of the second staging round takes lane 63's
             dword of the first / one that begins at region offset 1010..1018 behind four other letters at 1004..1007 (lane 62's dword)
  h     a repeat that ends at B, a non-letter ON B     c0 c1 c2 c3   a non-letter at B - 129 (outside chunk k's region: k stays on the sift
  sn0 sn1    (c >= 1024) a non-letter at region offset       stages), B - 128 (its first byte: k is walked), B - 1, B, a repeat next to each
             1023 / 1024, a repeat next to it
The kinds with a non-letter lie in contigs of their own, each alone in [B - c - 140, B + 2 c + 10): every other chunk there, and every chunk
of the contigs that hold the letters-only kinds, is a chunk of plain letters for every chunk size — it stays on the sift stages.
Inside a chunk, once per case: repeats that straddle 32, 64 and 1024 of a contig's first chunk (t32_0 t64_0 s_0 s2_0; no halo there); an
array of 400 bases at contig offset 0 (dpin), one that runs into the contig's partial last tile (dpout), one dense over whole tiles (dpdp),
arrays with 2 % substitutions (gaps) and one of 4300 bases across three default chunks (long); from T = 21 on a contig of three pieces that
leave gaps of 2, 4 and 6-7 between sifted positions in tiles that are stepped through (gapfix: see gap_ctg()).
Contigs of 0, 1, 2, 3, W - 1, W, W + 1, 63, 64, 65, 127, 128, 129 and, per chunk size, c - 1, c, c + 1, c + 15, c + 16, c + 17, 2 c, 2 c + 1
bases: up to 66 bases one whole array, beyond that ending flush with an array.  Single IUPAC letters lie outside every neighbourhood.

twin(): 4.5 Mbases of random sequence with the border kinds at every 50th default border (the product twin of the one-wave test).
cap_dense() / cap_exact(rows): the row capacity of a chunk, cap = max(16, 1792 / 32) = 56: homopolymers of 5 bases every 12 at (5, 7), and at
(30, 16), which leaves random sequence almost unmasked, one chunk with exactly `rows` intervals under the recording rule (rows_per_chunk())
and an interval that starts exactly at that chunk's end - W, which the next chunk records.

Measured (`python tests/sift_cases.py`, the CPU oracle alone on one core of a server CPU; aim: 2 s per case, 60 s for the module):
  default chunk, one assembly per pair: 116-121 kbases in 25-28 contigs, 82-87 default chunks, 29-30 plants; oracle seconds / intervals:
    (20,64) 0.16 / 74   (5,4) 0.00 / 1191   (5,7) 0.00 / 1561   (12,34) 0.04 / 358   (10,35) 0.03 / 396   (20,65) 0.15 / 77   (20,66) 0.27 / 78
    (79,66) 0.11 / 60   (80,66) 0.10 / 60   (100,64) 0.14 / 57   (319,66) 0.00 / 54   (320,66), (5,3), (100000,64) 0.00 / 0
  the seven run-time sizes, one assembly per pair: 645-647 kbases in 82-85 contigs, 141-142 plants, 417-421 default chunks:
    (20,64) 0.39 / 348   (5,7) 0.02 / 8664   (20,66) 0.37 / 348   (80,66) 0.21 / 245
  twin (20,64): 4 503 051 bases in 3 contigs, 2515 default chunks, 48 plants: 0.14 s / 944; the fullest chunk holds 3 rows
  cap_dense (5,7): 23 370 bases, 14 chunks, the fullest holds 154 rows; cap_exact(56) / (57) at (30,16): 23 612 bases, 15 chunks, 257 / 259 intervals
  total 2.1 s.  The oracle is far inside the aim, so nothing was cut: the plants are 60-110 bases (69-110 at T = 319, where only a homopolymer of
  66 bases or more is masked), the arrays 400, 600 and 4300.
"""
import functools
import sys
import time

import numpy as np

import oracle_bind as ob

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
OTHER = np.frombuffer(b"NNNnRYKMSWBDHVryk", dtype=np.uint8)      # N and IUPAC letters: all of them 4 in seq_nt4_table

CHUNK = 1792                                                     # SIFT_CHUNK_DEFAULT (sdust_sift.hpp): what the product runs
RT_CHUNKS = (256, 320, 1024, 1920, 1984, 3008, 3968)             # the run-time-size build at its own borders
PAIRS = [(20, 64), (5, 4), (5, 7), (12, 34), (10, 35), (20, 65), (20, 66), (79, 66), (80, 66), (100, 64), (319, 66)]
EMPTY = [(320, 66), (5, 3), (100000, 64)]                        # no interval can exist
RT_PAIRS = [(20, 64), (5, 7), (20, 66), (80, 66)]
SMALL_LENS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)

CLEAN_KINDS = ("a", "b1", "b2", "f", "g", "case", "r0", "r1", "r2", "t32", "t64")
DIRTY_KINDS = ("h", "c0", "c1", "c2", "c3")
ONCE_KINDS = {"t32_0", "t64_0", "s_0", "s2_0", "dpin", "dpout", "dpdp", "gaps", "long"}


def _repeat(rng, n, p, subst):
    """n bases of a random unit of p letters (no homopolymer unless p = 1), with about 2 % substitutions when asked"""
    while True:
        u = ACGT[rng.integers(0, 4, size=p)]
        if p == 1 or len(set(u.tolist())) > 1:
            break
    r = np.resize(u, n).copy()
    if subst and n >= 20:
        pos = rng.choice(n, size=max(1, n // 50), replace=False)
        r[pos] = ACGT[(np.searchsorted(ACGT, r[pos]) + rng.integers(1, 4, size=len(pos))) % 4]
    return r


def _pick(rng, T, W, n_lo=60, n_hi=110):
    """length and period of a planted repeat that the pair masks: a period-p array of k words scores about k / (2 p) per word, and k is at
    most the window's W - 2: p <= 5 k / (1.3 T), at most k / 2 (every word at least twice in the window) and at most 7"""
    n = int(rng.integers(n_lo, n_hi + 1))
    k = min(n, W) - 2
    return n, int(rng.integers(1, max(1, min(7, k // 2, int(5 * k / (1.3 * max(T, 1))))) + 1))


def _first_diff(got, exp):
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            return "interval %d: device %r, expected %r" % (i, g, e)
    return "device %d intervals, expected %d; the first one side lacks: %r" % (len(got), len(exp), (got + exp)[min(len(got), len(exp)):][:1])


def t_eff(T, W):
    """the T the plants are sized for: the pair's own, or, where nothing can be masked, the largest at which the window still masks"""
    return max(1, min(T, 5 * (W - 2) - 1))


def _pick_sift(rng, T, W):
    """as _pick(), and long enough that a homopolymer of that length is masked (more than T / 5 words)"""
    te = t_eff(T, W)
    return _pick(rng, te, W, max(60, min(110, te // 5 + 6)), 110)


def _pmax(T, W):
    k = W - 2
    return max(1, min(7, k // 2, int(5 * k / (1.3 * t_eff(T, W)))))


def _array(rng, T, W, n, subst=0.0, p=None):
    """an array of n bases whose period the pair masks; subst: the fraction of substituted bases"""
    r = _repeat(rng, n, p or int(rng.integers(1, _pmax(T, W) + 1)), False)
    if subst:
        m = rng.random(n) < subst
        r[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
    return r


def _other(rng, n=1):
    return OTHER[rng.integers(0, len(OTHER), size=n)]


def _not(rng, *letters):
    return np.array([[x for x in ACGT.tolist() if x not in letters][int(rng.integers(0, 4 - len(set(letters))))]], dtype=np.uint8)


def plant(rng, T, W, kind, B, halo=128):
    """-> (pieces [(position, bytes)], spans the oracle must mask, slack): kind at border B (halo = 0: B is a contig's base 0, for t and s)"""
    n, p = _pick_sift(rng, T, W)
    sub = T <= 20 and W >= 34 and kind not in ("a", "case", "r0", "r1", "r2") and bool(rng.integers(0, 2))
    rep = _repeat(rng, n, p, sub)
    r1k = 1024 - halo                                   # region offset 1024
    if kind in ("a", "case", "t32", "t64", "s"):
        at = B + {"a": 0, "case": 0, "t32": 32, "t64": 64, "s": r1k}[kind]
        x = int(rng.integers(1, n if halo else min(n, at + 1)))      # (a first chunk: nothing in front of base 0)
        return [(at - x, rep)], [(at - x, at - x + n)], 0
    if kind == "b1":
        return [(B - n, rep)], [(B - n, B)], 0
    if kind == "b2":
        return [(B, rep)], [(B, B + n)], 0
    if kind == "f":
        g1, g2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        n2 = _pick_sift(rng, T, W)[0]
        r = _repeat(rng, n + g1 + g2 + n2, p, sub)
        r[n:n + g1 + g2] = ACGT[rng.integers(0, 4, size=g1 + g2)]
        return [(B - g1 - n, r)], [(B - g1 - n, B - g1), (B + g2, B + g2 + n2)], 0
    if kind == "g":
        x = B - W + n // 2
        two = rng.permutation(4)[:2]
        return [(x - n, np.full(n, ACGT[two[0]])), (x, np.full(n, ACGT[two[1]]))], [(x - n, x), (x, x + n)], 0
    if kind in ("r0", "r1", "r2"):
        s = B - W + {"r0": -1, "r1": 0, "r2": 1}[kind]
        return [(s - 1, _not(rng, rep[0], rep[p - 1])), (s, rep)], [(s, s + n)], 0
    if kind == "s2":
        s = B + r1k - 14 + int(rng.integers(0, 9))      # region offsets 1010 .. 1018
        return [(B + r1k - 20, np.repeat(_not(rng, rep[B + r1k - 4 - s]), 4)), (s, rep)], [(s, s + n)], 0
    if kind == "h":
        return [(B - n, rep), (B, _other(rng))], [(B - n, B)], 0
    if kind in ("c0", "sn0"):                           # the repeat ends at the non-letter
        x = B - 129 if kind == "c0" else B + r1k - 1
        return [(x - n, rep), (x, _other(rng))], [(x - n, x)], 0
    # the repeat begins behind the non-letter: the window still holds the words from before it while the reference counts the window's start
    # from behind it (the stale-window quirk), and the interval is reported up to W further right
    x = {"c1": B - 128, "c2": B - 1, "c3": B, "sn1": B + r1k}[kind]
    return [(x, _other(rng)), (x + 1, rep)], [(x + 1, x + 1 + n)], W


class _Case:
    pass


def kinds_for(c):
    """the border kinds every case holds for chunk size c"""
    return set(CLEAN_KINDS + DIRTY_KINDS) | ({"s", "s2", "sn0", "sn1"} if c >= 1024 else set())


def ctg_lens(W, cvals):
    out = list(SMALL_LENS) + [W - 1, W, W + 1]
    for c in cvals:
        out += [c - 1, c, c + 1, c + 15, c + 16, c + 17, 2 * c, 2 * c + 1]
    return sorted(set(out))


def _oracle(k):
    t0 = time.perf_counter()
    k.per_ctg = [[(int(r) >> 32, int(r) & 0xFFFFFFFF) for r in ob.sdust(s, k.T, k.W)] for s in k.seqs]
    k.oracle_s = time.perf_counter() - t0
    k.exp = [(ci, a, b) for ci, iv in enumerate(k.per_ctg) for a, b in iv]
    return k


@functools.lru_cache(maxsize=None)
def case(T, W, cvals=(CHUNK,)):
    """-> the assembly planted for the chunk sizes cvals, what was planted where, and the oracle's intervals"""
    rng = np.random.default_rng(91_000 + 131 * W + (T % 9973) + 7 * len(cvals))
    CAP = 40_000
    clean, dirty = [], []                               # contigs under construction: {"busy": [(lo, hi)], "pieces": [(pos, bytes)]}
    placed = []

    def free(ctg, lo, hi):
        return all(hi <= a or lo >= b for a, b in ctg["busy"])

    def place(pool, c, lo, hi, cap):
        """a border B = k c of a contig of `pool` with [B + lo, B + hi) to itself"""
        for ctg in pool + [None]:
            if ctg is None:
                ctg = {"busy": [(0, 1400)], "pieces": []}          # (the first 1400 bases: the kinds of a contig's first chunk)
                pool.append(ctg)
            for k in range(1, cap // c + 1):
                B = k * c
                if B + lo >= 0 and B + hi <= cap - 600 and free(ctg, B + lo, B + hi):
                    ctg["busy"].append((B + lo, B + hi))
                    return ctg, B
        raise AssertionError("no room for a border of chunk size %d" % c)

    for c in cvals:
        for kind in sorted(kinds_for(c)):
            if kind in CLEAN_KINDS + ("s", "s2"):
                mid = 896 if kind in ("s", "s2") else 0
                ctg, B = place(clean, c, mid - 450, mid + 450, CAP)
                pool = "clean"
            else:
                ctg, B = place(dirty, c, -c - 140, 2 * c + 10, max(CAP, 8 * c))
                pool = "dirty"
            pieces, spans, slack = plant(rng, T, W, kind, B)
            if kind == "case":
                ctg.setdefault("lower", []).append((B - 300, B + 300))
            ctg["pieces"] += pieces
            placed.append({"c": c, "kind": kind, "pool": pool, "ctg_obj": ctg, "B": B, "spans": spans, "slack": slack})
    # the first chunk of three letters-only contigs: 32 and 64, 1024, 1010 (no halo: region offset = position)
    while len(clean) < 3:
        clean.append({"busy": [(0, 1400)], "pieces": []})
    for ctg, kinds in zip(clean, (("t32", "s"), ("t64",), ("s2",))):
        for kind in kinds:
            pieces, spans, slack = plant(rng, T, W, kind, 0, halo=0)
            ctg["pieces"] += pieces
            placed.append({"c": 0, "kind": kind + "_0", "pool": "clean", "ctg_obj": ctg, "B": 0, "spans": spans, "slack": 0})

    def finish(ctg, is_dirty):
        top = max(b for _, b in ctg["busy"])
        ln = top + int(rng.integers(700, 1500))
        s = ACGT[rng.integers(0, 4, size=ln)].copy()
        if is_dirty:                                    # single IUPAC letters, none within W in front of a neighbourhood
            for q in rng.integers(0, ln, size=6):
                if free(ctg, q - 10, q + W + 10):
                    s[q] = _other(rng)[0]
        for pos, arr in ctg["pieces"]:
            s[pos:pos + len(arr)] = arr
        for lo, hi in ctg.get("lower", []):
            seg = s[lo:hi]
            seg[np.isin(seg, ACGT)] |= 0x20
        n = _pick_sift(rng, T, W)[0]
        s[ln - n:] = _array(rng, T, W, n)               # ends flush with an array
        return s
    bigs = [(ctg, finish(ctg, False)) for ctg in clean] + [(ctg, finish(ctg, True)) for ctg in dirty]

    # the arrays: dp-in at contig offset 0, dp-dp, gaps, dp-out into the partial last tile; long across three default chunks
    def arr_ctg():
        parts, spans, pos = [], {}, 0

        def add(name, a):
            nonlocal pos
            if name:
                spans.setdefault(name, []).append((pos, pos + len(a)))
            parts.append(a)
            pos += len(a)
        add("dpin", _array(rng, T, W, 400))
        add(None, ACGT[rng.integers(0, 4, size=1500)])
        add("dpdp", _array(rng, T, W, 400))
        for p in [q for q in (1, 2, 3, 5) if q <= _pmax(T, W)]:
            add(None, ACGT[rng.integers(0, 4, size=700)])
            add("gaps", _array(rng, T, W, 600, 0.02, p))
        add(None, ACGT[rng.integers(0, 4, size=1300)])
        add(None, ACGT[rng.integers(0, 4, size=(37 - pos - 400) % 64)])
        add("dpout", _array(rng, T, W, 400))
        return np.concatenate(parts), spans

    def long_ctg():
        s = ACGT[rng.integers(0, 4, size=6100)].copy()
        s[1000:5300] = _array(rng, T, W, 4300)
        s[6000:] = _array(rng, T, W, 100)
        return s, {"long": [(1000, 5300)]}

    def gap_ctg():
        """T > 20: the sieve passes positions deep inside arrays only, and the diverged arrays above leave no short gaps between sifted
        positions.  Three pieces, each ending early in a tile (fewer than 24 sifted positions: the tile is stepped through, it is no dp tile):
        A x 30, (CA) x 18, AA — the words ACA (common), CAA (new), AAA (common again): a gap of 2; A x 85 with one other letter and A x 88
        with two: 3 or 5 broken words, then the positions at which the partial sums of L1 still fail: gaps of 4 and of 6-7 (T = 319: 7 and
        12, and nothing at the first piece — no shorter gap exists there, see test_product_default_chunking)"""
        s = ACGT[rng.integers(0, 4, size=1500)].copy()
        A, C, G = ACGT[0], ACGT[1], ACGT[2]
        s[320 - 31], s[320 + 38] = G, G
        s[320 - 30:320] = A
        s[320:320 + 36] = np.resize(np.array([C, A], dtype=np.uint8), 36)
        s[320 + 36:320 + 38] = A
        for q, subs, end in ((704, (10,), 21), (1088, (10, 12), 24)):
            s[q - 65], s[q + end] = G, G
            s[q - 64:q + end] = A
            for x in subs:
                s[q + x] = C
        s[1400:] = _array(rng, T, W, 100)
        return s, {"gapfix": [(704 - 64, 704 + 10)]}
    specials = [arr_ctg(), long_ctg()] + ([gap_ctg()] if t_eff(T, W) > 20 else [])

    def small(n):
        if n <= 66:
            return _repeat(rng, n, min(1 + n % 2, _pmax(T, W)), False) if n else np.zeros(0, np.uint8)
        t = ACGT[rng.integers(0, 4, size=n)].copy()
        m = min(n, _pick_sift(rng, T, W)[0])
        t[n - m:] = _array(rng, T, W, m)
        return t
    smalls = [small(n) for n in ctg_lens(W, cvals)]
    # the order: a special or a big contig, then a few of the short ones
    seqs, where = [], {}
    heads = [(None, s, sp) for s, sp in specials] + [(ctg, s, None) for ctg, s in bigs]
    per = (len(smalls) + len(heads) - 1) // len(heads)
    for i, (ctg, s, sp) in enumerate(heads):
        if ctg is not None:
            where[id(ctg)] = len(seqs)
        else:
            for name, spans in sp.items():
                placed.append({"c": 0, "kind": name, "pool": "array", "ctg": len(seqs), "B": 0, "spans": spans, "slack": 0})
        seqs.append(s)
        seqs += smalls[i * per:(i + 1) * per]
    k = _Case()
    k.T, k.W, k.cvals = T, W, cvals
    k.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    k.placed = [{kk: v for kk, v in dict(pl, ctg=pl["ctg"] if "ctg" in pl else where[id(pl["ctg_obj"])]).items() if kk != "ctg_obj"} for pl in placed]
    return _oracle(k)


@functools.lru_cache(maxsize=None)
def other_exp(T, W, T2, W2):
    """the oracle's intervals of the default-chunk assembly of (T, W) at ANOTHER pair: what a second pair on the same resident assembly gives"""
    return [(ci, int(r) >> 32, int(r) & 0xFFFFFFFF) for ci, s in enumerate(case(T, W).seqs) for r in ob.sdust(s, T2, W2)]


def n_chunks(seqs, c=CHUNK):
    return sum((len(s) + c - 1) // c for s in seqs)


def check(k):
    """the self-checks of a case: every kind is there for every chunk size, the contig lengths are there, and the oracle reports an interval
    over every planted repeat (an interval over the border itself where a repeat straddles it); nothing at all for the pairs of EMPTY"""
    assert sorted(set(len(s) for s in k.seqs) & set(ctg_lens(k.W, k.cvals))) == ctg_lens(k.W, k.cvals)
    for c in k.cvals:
        assert {pl["kind"] for pl in k.placed if pl["c"] == c} == kinds_for(c), (c, k.T, k.W)
    assert {pl["kind"] for pl in k.placed if pl["c"] == 0} == ONCE_KINDS | ({"gapfix"} if t_eff(k.T, k.W) > 20 else set())
    for pl in k.placed:                                 # the chunks around a letters-only kind hold letters only, for every chunk size
        s = k.seqs[pl["ctg"]]
        if pl["pool"] != "dirty":
            assert np.isin(s & 0xDF, ACGT).all(), pl
        elif pl["c"]:
            c, B = pl["c"], pl["B"]
            assert int((~np.isin(s[B - c - 128:B + 2 * c] & 0xDF, ACGT)).sum()) == 1, pl
    if (k.T, k.W) in EMPTY:
        assert k.exp == [], (k.T, k.W, k.exp[:3])
        return
    assert (k.T, k.W) in PAIRS
    for pl in k.placed:
        iv = k.per_ctg[pl["ctg"]]
        for s, e in pl["spans"]:
            assert any(a < e + pl["slack"] and b > s for a, b in iv), ("the oracle masks nothing over a planted repeat", k.T, k.W, pl)
        if pl["kind"] in ("a", "case"):
            assert any(a < pl["B"] < b for a, b in iv), ("no interval over the border", k.T, k.W, pl)
        if pl["kind"] == "g":
            x = pl["spans"][0][1]
            assert any(a < x - 20 and b > x + 20 for a, b in iv), ("the two arrays are not one interval", k.T, k.W, pl)
    for ci, s in enumerate(k.seqs):                     # every longer contig ends with an array
        if len(s) >= 127:
            assert any(b >= len(s) - 1 for _, b in k.per_ctg[ci]), ("nothing masked at a contig's end", k.T, k.W, ci, len(s))


@functools.lru_cache(maxsize=None)
def twin(T=20, W=64):
    """4.5 Mbases of random sequence in three contigs (2500 default chunks: several for each of the waves a 10 % share leaves the kernel),
    the border kinds in turn at every 50th default border"""
    rng = np.random.default_rng(4711)
    kinds = sorted(kinds_for(CHUNK))
    seqs, placed = [], []
    for ci in range(3):
        ln = 1_500_000 + 1000 * ci + 17
        s = ACGT[rng.integers(0, 4, size=ln)].copy()
        for j, B in enumerate(range(50 * CHUNK, ln - 2 * CHUNK, 50 * CHUNK)):
            kind = kinds[(j + 5 * ci) % len(kinds)]
            pieces, spans, slack = plant(rng, T, W, kind, B)
            for pos, arr in pieces:
                s[pos:pos + len(arr)] = arr
            placed.append({"c": CHUNK, "kind": kind, "pool": "twin", "ctg": ci, "B": B, "spans": spans, "slack": slack})
        seqs.append(s)
    k = _Case()
    k.T, k.W, k.cvals = T, W, (CHUNK,)
    k.seqs, k.placed = seqs, placed
    _oracle(k)
    for pl in k.placed:
        for s, e in pl["spans"]:
            assert any(a < e + pl["slack"] and b > s for a, b in k.per_ctg[pl["ctg"]]), ("the oracle masks nothing over a planted repeat", pl)
    return k


def rows_per_chunk(k, c=CHUNK):
    """{(contig, chunk): rows} by the recording rule of a chunk of plain letters: chunk j = [B, B + c) records the intervals whose start lies in
    [B - W, B + c - W); a contig's first chunk from 0, its last one everything that is left"""
    rows = {}
    for ci, iv in enumerate(k.per_ctg):
        last = max(0, (len(k.seqs[ci]) + c - 1) // c - 1)
        for a, _ in iv:
            j = min(last, (a + k.W) // c)
            rows[(ci, j)] = rows.get((ci, j), 0) + 1
    return rows


CAP_ROWS = max(16, CHUNK // 32)                          # sdust_asm_impl(): rows per chunk of the first attempt


@functools.lru_cache(maxsize=None)
def cap_dense():
    """(5, 7): homopolymers of 5 bases every 12 — far more rows per chunk than the capacity"""
    rng = np.random.default_rng(57)
    k = _Case()
    k.T, k.W, k.cvals = 5, 7, (CHUNK,)
    k.seqs = []
    for ln in (9 * CHUNK + 77, CHUNK - 3, 3 * CHUNK):
        s = ACGT[rng.integers(0, 4, size=ln)].copy()
        if ln != 3 * CHUNK:
            for p in range(7, ln - 5, 12):
                s[p:p + 5] = ACGT[(p // 12) % 4]
        k.seqs.append(s)
    k.placed = []
    return _oracle(k)


CAP_AT = (0, 5)                                          # the designated chunk of cap_exact(): contig 0, chunk 5


@functools.lru_cache(maxsize=None)
def cap_exact(rows):
    """(30, 16), letters only: chunk CAP_AT holds exactly `rows` intervals by the recording rule, every other chunk fewer; one more interval
    starts exactly at that chunk's end - W, the first start the NEXT chunk records"""
    T, W, c, d = 30, 16, CHUNK, CAP_AT[1]
    for seed in range(40):
        rng = np.random.default_rng(3016 + 100 * rows + seed)
        s = ACGT[rng.integers(0, 4, size=12 * c + 300)].copy()

        def homo(p):
            s[p:p + 10] = _not(rng, s[p - 1], s[p + 10])[0]
        for i in range(rows):
            homo(d * c - W + 20 + 30 * i)
        homo((d + 1) * c - W)
        for j in range(12):
            if j not in (d, d + 1):
                for i in range(20):
                    homo(j * c + 100 + 70 * i)
        k = _Case()
        k.T, k.W, k.cvals = T, W, (c,)
        k.seqs = [s, ACGT[rng.integers(0, 4, size=c + 16)].copy()]
        k.placed = []
        _oracle(k)
        got = rows_per_chunk(k)
        if got.get(CAP_AT) == rows and max(v for kk, v in got.items() if kk != CAP_AT) < rows and ((d + 1) * c - W) in [a for a, _ in k.per_ctg[0]]:
            return k
    raise AssertionError("no seed gives exactly %d rows" % rows)


if __name__ == "__main__":      # the oracle's time per case (no device needed): what the figures in the module docstring were measured with
    total = 0.0
    todo = [(T, W, (CHUNK,)) for T, W in PAIRS + EMPTY] + [(T, W, RT_CHUNKS) for T, W in RT_PAIRS]
    for T, W, cv in todo:
        k = case(T, W, cv)
        check(k)
        print("T %6d W %2d chunks %-8s oracle %5.2f s, %7d bases in %3d contigs, %5d default chunks, %5d intervals, %3d plants" % (
            T, W, "default:" if cv == (CHUNK,) else "%d sizes:" % len(cv), k.oracle_s, sum(map(len, k.seqs)), len(k.seqs), n_chunks(k.seqs), len(k.exp),
            len(k.placed)), flush=True)
        total += k.oracle_s
    for name, k in (("twin", twin()), ("cap_dense", cap_dense()), ("cap_exact(56)", cap_exact(56)), ("cap_exact(57)", cap_exact(57))):
        print("%-14s (%d, %d): oracle %5.2f s, %7d bases in %d contigs, %5d default chunks, %5d intervals, %3d plants, fullest chunk %d rows" % (
            name, k.T, k.W, k.oracle_s, sum(map(len, k.seqs)), len(k.seqs), n_chunks(k.seqs), len(k.exp), len(k.placed), max(rows_per_chunk(k).values())), flush=True)
        total += k.oracle_s
    print("total %.1f s" % total)
    sys.exit(0)
