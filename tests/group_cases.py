"""Planted inputs for the chunk groups of sd_sift (cornetto_amd/csrc/sdust_sift.hpp: SIFT_GROUP consecutive chunks per counter request, the
seam tile carried from one chunk of a group to the next) — CPU only, no device.  tests/test_sdust_groups_host.py checks the cases themselves,
tests/test_gpu_sdust_groups.py runs them on the device against the oracle's intervals kept here.  The small helpers are those of
tests/sift_cases.py.

A chunk is 1792 bases (sift_cases.CHUNK); the chunk table lists the contigs in order, so chunk i of the table is position i of the hand-out
order of a first call, and group g holds the chunks g G .. g G + G - 1.  Chunk i takes the seam over from chunk i - 1 ("carried") when
  i is not a multiple of G, both are chunks of one contig, and neither holds a byte other than a letter within [start - 128, end);
every other chunk redoes the two tiles in front of it.  carried(seqs, G) counts them by that rule.

assembly(T, W, G), one for every pair and group size, a few kbases per contig:
  layout   letters-only contigs of 1792, 1793, 3584, 3585, G 1792, G 1792 + 1 and (G + 1) 1792 + 5 bases, runs of contigs of 1, 63, 100 and 1792
           bases between them (a group spans contig borders), every longer one ending flush with an array
  seam     three contigs of G + 2 chunks: at EVERY border B inside them a feature that ends in / starts in / straddles the last 128 bases in
           front of B.  G + 1 consecutive borders: at least one seam that is redone (a group's first chunk) and one that is carried
  bytes    (dirty=True) three contigs with ONE byte that is no letter, in the second chunk j of a group: in its middle (j is walked, j + 1
           falls back to redoing its seam), 60 bases in front of its end (j and, through its halo, j + 1 are walked), at its first base (j is
           walked; j - 1 does not see it); a repeat right behind each of them
"""
import functools

import numpy as np

import oracle_bind as ob
import sift_cases as sc

CHUNK = sc.CHUNK
GROUPS = (2, 4, 8)                                      # the group sizes the host test checks the cases for
PAIRS = [(20, 64), (20, 66), (5, 7)]
SEAM_KINDS = ("ends_in", "starts_in", "straddles")
BYTE_KINDS = ("middle", "last128", "first")


def chunk_table(seqs, c=CHUNK):
    """-> [(contig, start, end)] in the order of the device's chunk table"""
    return [(ci, s, min(s + c, len(q))) for ci, q in enumerate(seqs) for s in range(0, len(q), c)]


def unclean(seqs, c=CHUNK):
    """-> a flag per chunk: a byte other than A/C/G/T (either case) within [start - 128, end)"""
    out = []
    for ci, s, e in chunk_table(seqs, c):
        seg = seqs[ci][max(0, s - 128):e]
        out.append(bool((~np.isin(seg & 0xDF, sc.ACGT)).any()))
    return out


def carried(seqs, G, c=CHUNK):
    """-> the table indices of the chunks that take their seam over from the chunk before, on a first call (hand-out order = table order)"""
    tab, bad = chunk_table(seqs, c), unclean(seqs, c)
    return [i for i, (ci, s, e) in enumerate(tab) if i % G and s > 0 and not bad[i] and not bad[i - 1]]


def closed_form(seqs, G, c=CHUNK):
    """letters only: every chunk that is neither the first of its contig nor the first of its group"""
    n, i = 0, 0
    for q in seqs:
        for j in range((len(q) + c - 1) // c):
            n += 1 if (j > 0 and i % G) else 0
            i += 1
    return n


class _Case:
    pass


def _ctg(rng, T, W, n):
    """n random bases; from 127 bases on ending flush with an array the pair masks"""
    s = sc.ACGT[rng.integers(0, 4, size=n)].copy()
    if n >= 127:
        m = sc._pick_sift(rng, T, W)[0]
        s[n - m:] = sc._array(rng, T, W, m)
    return s


def seam_feature(rng, T, W, kind, B):
    """-> (position, bytes): a feature against the last 128 bases in front of the border B"""
    n = sc._pick_sift(rng, T, W)[0]
    if kind == "ends_in":                               # starts in front of B - 128, ends inside [B - 128, B)
        e = int(rng.integers(20, 120))
        return B - 128 + e - n, sc._array(rng, T, W, n)
    if kind == "starts_in":                             # starts inside, runs across B
        x = int(rng.integers(10, min(n, 120) - 5))
        return B - x, sc._array(rng, T, W, n)
    return B - 160, sc._array(rng, T, W, 200)           # over all 128 of them and across B


@functools.lru_cache(maxsize=None)
def assembly(T, W, G, dirty=True):
    rng = np.random.default_rng(77_000 + 131 * W + (T % 9973) + 17 * G)
    seqs, seams, planted_bytes = [], [], []

    def n_before():
        return sum((len(s) + CHUNK - 1) // CHUNK for s in seqs)

    shorts = (1, 63, 100, 1792)
    for i, ln in enumerate((1792, 1793, 3584, 3585, G * CHUNK, G * CHUNK + 1, (G + 1) * CHUNK + 5)):
        seqs.append(_ctg(rng, T, W, ln))
        seqs += [_ctg(rng, T, W, shorts[(i + j) % 4]) for j in range(1 + i % 3)]
    for kind in SEAM_KINDS:
        s = _ctg(rng, T, W, (G + 2) * CHUNK - 300)
        for j in range(1, G + 2):
            pos, arr = seam_feature(rng, T, W, kind, j * CHUNK)
            s[pos:pos + len(arr)] = arr
            seams.append({"kind": kind, "ctg": len(seqs), "B": j * CHUNK, "chunk": n_before() + j, "span": (pos, pos + len(arr))})
        seqs.append(s)
        seqs.append(_ctg(rng, T, W, 100))
    if dirty:
        for kind in BYTE_KINDS:
            i0 = n_before()
            j = next(l for l in range(1, G + 1) if (i0 + l) % G == 1)          # the second chunk of a group
            s = _ctg(rng, T, W, (j + 3) * CHUNK + 40)
            B = j * CHUNK
            at = {"middle": B + 900, "last128": B + CHUNK - 60, "first": B}[kind]
            pieces, _, _ = sc.plant(rng, T, W, "c3", at)                         # the byte at `at`, a repeat behind it
            for pos, arr in pieces:
                s[pos:pos + len(arr)] = arr
            planted_bytes.append({"kind": kind, "ctg": len(seqs), "at": at, "chunk": i0 + j})
            seqs.append(s)
    k = _Case()
    k.T, k.W, k.G = T, W, G
    k.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    k.seams, k.bytes = seams, planted_bytes
    k.per_ctg = [[(int(r) >> 32, int(r) & 0xFFFFFFFF) for r in ob.sdust(s, T, W)] for s in k.seqs]
    k.exp = [(ci, a, b) for ci, iv in enumerate(k.per_ctg) for a, b in iv]
    return k


@functools.lru_cache(maxsize=None)
def other_exp(T, W, G, T2, W2):
    return [(ci, int(r) >> 32, int(r) & 0xFFFFFFFF) for ci, s in enumerate(assembly(T, W, G).seqs) for r in ob.sdust(s, T2, W2)]


def lost_seams(k):
    """the seams the planted bytes take away, named: chunk j is the second of its group, so the seam into it would have been carried; the seam
    into j + 1 is lost with it (G > 2: at G = 2, j + 1 begins a group), and behind a byte in j's last 128 bases the seam into j + 2 as well
    (G > 3)"""
    G, out = k.G, []
    for b in k.bytes:
        j = b["chunk"]
        out += [j] + ([j + 1] if (j + 1) % G else []) + ([j + 2] if b["kind"] == "last128" and (j + 2) % G else [])
    return sorted(out)


def check(k):
    """the self-checks of a case"""
    G, tab, bad = k.G, chunk_table(k.seqs), unclean(k.seqs)
    lens = [len(s) for s in k.seqs]
    for ln in (1792, 1793, 3584, 3585, G * CHUNK, G * CHUNK + 1, (G + 1) * CHUNK + 5, 1, 63, 100):
        assert ln in lens, ln
    # a group that spans a contig border, one that spans three contigs (G = 2: two)
    assert any(tab[i][0] != tab[i + 1][0] for i in range(len(tab) - 1) if (i + 1) % G)
    assert any(len({tab[i][0] for i in range(g, min(g + G, len(tab)))}) >= min(3, G) for g in range(0, len(tab), G))
    cy = set(carried(k.seqs, G))
    for kind in SEAM_KINDS:                             # every seam kind at a carried and at a redone seam, and the oracle masks it
        mine = [s for s in k.seams if s["kind"] == kind]
        assert any(s["chunk"] in cy for s in mine) and any(s["chunk"] % G == 0 for s in mine), kind
        for s in mine:
            assert tab[s["chunk"]][:2] == (s["ctg"], s["B"])
            lo, hi = s["span"]
            assert lo < s["B"] and hi > s["B"] - 128
            assert any(a < hi and b > lo for a, b in k.per_ctg[s["ctg"]]), ("the oracle masks nothing over a seam feature", k.T, k.W, s)
    letters = assembly(k.T, k.W, G, dirty=False)
    assert not any(unclean(letters.seqs)) and len(carried(letters.seqs, G)) == closed_form(letters.seqs, G) > 0
    if not k.bytes:
        assert not any(bad)
        return
    assert [s.tobytes() for s in k.seqs[:len(letters.seqs)]] == [s.tobytes() for s in letters.seqs]
    n_letters = len(chunk_table(letters.seqs))
    for b in k.bytes:
        j = b["chunk"]
        assert j % G == 1 and tab[j][0] == b["ctg"] and tab[j][1] <= b["at"] < tab[j][2]
        assert tab[j - 1][0] == tab[j + 2][0] == b["ctg"]
        assert not np.isin(k.seqs[b["ctg"]][b["at"]] & 0xDF, sc.ACGT)
        assert bad[j] and not bad[j - 1] and bad[j + 1] == (b["kind"] == "last128") and not bad[j + 2]
    assert sum(bad) == 4
    # the count with the bytes = the closed form of the same layout in letters, less the seams named
    assert sorted(set(i for i in range(n_letters, len(tab)) if i % G and tab[i][1] > 0) - cy) == lost_seams(k)
    assert len(cy) == closed_form(k.seqs, G) - len(lost_seams(k))
