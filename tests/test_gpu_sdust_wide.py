"""The sdust kernels OFF the fast path, across chunk seams: sdust_kernel_g (258 <= W <= 1026, state in global memory), sdust_kernel<256>
(67 <= W <= 257, byte counters in LDS) and sdust_kernel<64> where the fast path does not take the pair (T < 5 or T > 100000), each against
the CPU oracle (oracle/oracle.c) with exact equality of (ctg, start, finish), at forced decompositions whose borders are planted with repeats.

Section 1 (test_seams_vs_oracle, test_overflow_retry_vs_oracle): one assembly per (T, W), built by _case(): for EVERY chunk size of _chunks(W)
it holds, at borders k * c of that size, a repeat straddling the border (a), one ending exactly at it (b1) and one starting exactly at it (b2),
one inside the 2 W look-back with a run of non-bases between it and the border (c), two repeats closer than W on either side of the border (f),
one that ends at the border with a non-base on the border (h: saved at the chunk's very first step) and, up to W = 257, two arrays end to end
whose touching intervals two different lanes record (g);
plus repeats flush with a contig's start (d) and end (e), lower case, IUPAC letters, bytes 0..3, and contigs of 0, 1, 2, W - 1, W, W + 1 and 13
bases.  The oracle runs once per (T, W); every chunk size of the pair then runs the same assembly on the device.  A case asserts first that the
oracle reported an interval over every repeat planted for its chunk size, so an emptied case fails instead of passing.  The exception is
T > 100000 at W <= 66: 10 r <= 10 * C(62, 2) = 18910 < T l for every l >= 1, so no interval can exist at all (:112 of the reference never
holds), and those cases assert that oracle and device both return none.

Section 2 (test_decomposition_invariance): at T = 20 and W in {100, 257, 258, 530, 1026} random sequence is itself masked and the oracle needs
minutes, so there the forced decompositions are compared with the one-chunk-per-contig run of the same kernel (u = 0, rec_from = 0, nothing to
stitch: the sequential algorithm, which section 1 pins to the oracle).  This is WEAKER than the oracle comparison: an error common to every
decomposition (in the recurrence itself) passes.  What it isolates is the seam logic alone: where a lane starts (the walk back over W - 2 word
emissions from chunk start - 2 W), that the speculative state equals the sequential one from the chunk start on, what a lane records (rec_from),
the sentinel step of a contig's last chunk, the stitch of the chunk lists, and the chunk table cached with the resident assembly (a->sd_chunk).

Section 3: the product build at its default decomposition, the drop-ins cornetto_sdust() / cornetto_sdust_core(), and the CLI.

What the budget was measured against (the CPU oracle alone, one core of an Intel Xeon server, `python tests/test_gpu_sdust_wide.py`, which
prints the figures below; aim: 5 s per parametrised case, 3 min for the module).  From W = 258 on every chunk size has an assembly of its own
(nine per pair); slowest case / sum over the pair's nine:
  sdust_kernel_g     (40,258) 0.4 / 2.9 s  (70,514) 2.1 / 11.4 s  (70,515) 1.5 / 9.7 s  (80,530) 1.6 / 11.2 s  (110,777) 2.7 / 17.3 s
                     (150,1025) 3.8 / 23.5 s  (150,1026) 4.9 / 26.1 s
  sdust_kernel<256>  one assembly per pair: (20,67) 0.2 s  (20,100) 0.7 s  (25,130) 1.2 s  (30,200) 2.1 s  (40,256) 3.2 s  (40,257) 3.4 s
  sdust_kernel<64>   (0,64) 0.3 s  (1,5) 0.0 s  (2,33) 0.1 s  (4,66) 0.3 s  (3,64) 1.1 s  (100001,64) 0.0 s  (1<<20,20) 0.0 s
  total 115 s; the three overflow inputs and the two letters-only assemblies of the CLI case add about 2 s.
Planted repeats are 60..110 bases, 60..80 from W = 200 on: it is the repeat bases, not the seams, that were cut to stay inside the budget (the
oracle needs about 0.25 s per planted repeat at W >= 514, and its time on one array grows with the cube of min(length, W)).
The per-chunk capacity the overflow cases exceed: cap = max(16, chunk / 32) rows (sdust_asm_impl), raised to whatever the handle's row
workspace already holds — hence a fresh handle per case.  sdust_kernel<64> and <256> exceed the natural 16 of a 520-base chunk (42 and 21
intervals per chunk); sdust_kernel_g cannot (17 intervals more than W >= 258 apart do not fit into the 543 bases up to which cap stays 16), so
its case pins cap to 3 with the development switch CORNETTO_SDUST_CAP and plants 7 repeats per chunk of 10 W.
The largest cases: sdust_kernel_g (40, 258) at chunk 128: 73 029 bases in 11 contigs, 578 chunks = 578 lanes in 10 workgroups;
sdust_kernel<256> (40, 257) at chunk 128: 139 075 bases, 1094 chunks; sdust_kernel<64> (1, 5) at chunk 17: 73 810 bases, 4348 chunks.
"""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_bind as ob
from helpers import fmt_sdust, ref_sdust
from sift_cases import ACGT, OTHER, _first_diff, _pick, _repeat      # (shared with the planted cases of the fast path)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFSO = os.path.join(ROOT, "oracle", "_ref", "libcornetto_ref.so")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "cornetto")

K_G = [(40, 258), (70, 514), (70, 515), (80, 530), (110, 777), (150, 1025), (150, 1026)]
K_256 = [(20, 67), (20, 100), (25, 130), (30, 200), (40, 256), (40, 257)]
K_64 = [(0, 64), (1, 5), (2, 33), (4, 66), (100001, 64), (1 << 20, 20), (3, 64)]          # (3, 64): on two-letter contigs
PAIRS = K_G + K_256 + K_64
RICH_W = [100, 257, 258, 530, 1026]


@pytest.fixture(scope="module")
def acc():
    import cornetto_amd
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def _default_chunk(W):
    """sdust_asm_impl() off the fast path, assemblies far below one chunk per resident lane: 1536 bases, and at least 32 W from W = 258 on"""
    return 1536 if W <= 257 else 32 * W


def _chunks(W):
    """"0" (the default) and about W / 2, W, 3 W, 10 W, each once as a value that is no multiple of 64 and once as one that is"""
    out = ["0"]
    for x in (W // 2, W, 3 * W, 10 * W):
        for v in (max(17, x | 1), max(64, (x + 32) // 64 * 64)):
            if str(v) not in out:
                out.append(str(v))
    return out


def _chunk_value(chunk, W):
    return _default_chunk(W) if int(chunk) <= 0 else max(16, int(chunk))


def _n_chunks(seqs, c):
    return sum((len(s) + c - 1) // c for s in seqs)


class _Case:
    pass


def _all_cvals(W):
    out = []
    for ch in _chunks(W):
        if _chunk_value(ch, W) not in out:
            out.append(_chunk_value(ch, W))
    return tuple(out)


def _case_for(T, W, chunk, codes=True):
    """the assembly a (T, W, chunk size) case runs: up to W = 257 one per pair, planted for every chunk size of the pair; from W = 258 on, where
    the oracle needs about a quarter of a second per planted repeat, one per chunk size"""
    return _case(T, W, _all_cvals(W) if W <= 257 else (_chunk_value(chunk, W),), codes)


@functools.lru_cache(maxsize=None)
def _case(T, W, cvals, codes=True):
    """-> the assembly planted for the chunk sizes cvals, what was planted where, and the oracle's intervals.  codes = False: letters only
    (for FASTA text)"""
    wide = W > 257
    rng = np.random.default_rng(77_000 + 131 * W + (T % 9973) + (cvals[0] if wide else 0))
    CAP = 84_000                                    # longest contig
    left, right = 3 * W + 300, W + 300              # what a planted border keeps to itself: its look-back and the repeats behind it
    big = [{"busy": [], "plants": []} for _ in range(3)]
    placed = []
    n_place = 0

    def free(ctg, lo, hi):
        return all(hi <= a or lo >= b for a, b in ctg["busy"])

    def pick():
        return _pick(rng, T, W, 60, 80 if W >= 200 else 110)         # (the oracle's time: the repeat bases, not the seams, are what is cut)

    def place(c):
        nonlocal n_place
        n_place += 1
        order = list(range(len(big)))
        order = order[n_place % 3:] + order[:n_place % 3] + [len(big)]      # (the last: a new contig)
        for ci in order:
            if ci == len(big):
                big.append({"busy": [], "plants": []})
            for k in range(1, CAP // c + 1):
                B = k * c
                if B - left < 300:
                    continue
                if B + right > CAP - 400:
                    break
                if free(big[ci], B - left, B + right):
                    big[ci]["busy"].append((B - left, B + right))
                    return ci, B
        raise AssertionError("no room for a border of chunk size %d" % c)

    for c in cvals:
        for kind in ("a", "b1", "b2", "c", "f", "h") + (() if wide else ("g",)):
            ci, B = place(c)
            n, p = pick()
            sub = bool(rng.integers(0, 2))
            spans = []
            if kind == "a":                          # straddles the border
                x = int(rng.integers(1, n))
                big[ci]["plants"].append((B - x, _repeat(rng, n, p, sub)))
                spans.append((B - x, B - x + n))
            elif kind == "b1":                       # ends exactly at the border
                big[ci]["plants"].append((B - n, _repeat(rng, n, p, sub)))
                spans.append((B - n, B))
            elif kind == "b2":                       # starts exactly at the border
                big[ci]["plants"].append((B, _repeat(rng, n, p, sub)))
                spans.append((B, B + n))
            elif kind == "c":                        # inside the 2 W look-back, non-bases between it and the border; more of them where the walk back counts words
                d, nn = int(rng.integers(3, 12)), int(rng.integers(1, 9))
                n = max(4, min(n, 2 * W - d - nn - 2))
                e = B - d - nn
                big[ci]["plants"].append((e - n, _repeat(rng, n, p, sub)))
                big[ci]["plants"].append((e, OTHER[rng.integers(0, len(OTHER), size=nn)]))
                big[ci]["plants"].append((min(B - 2 * W - W // 2 - 7, e - n - 5), OTHER[rng.integers(0, len(OTHER), size=int(rng.integers(1, 4)))]))
                spans.append((e - n, e))
            elif kind == "h":                        # ends at the border, a non-base ON the border: every interval is saved at the chunk's first step
                big[ci]["plants"].append((B - n, _repeat(rng, n, p, sub)))
                big[ci]["plants"].append((B, OTHER[rng.integers(0, len(OTHER), size=1)]))
                spans.append((B - n, B))
            elif kind == "g":
                # two homopolymers of different letters end to end: two intervals that touch, which the reference merges (:94-98).  The
                # first is saved about W behind its start, the second n later: with the border between the two times (and so for every
                # chunk size up to n) two lanes hold one each, and only the stitch can merge them
                x = B - W + n // 2
                two = rng.permutation(4)[:2]
                big[ci]["plants"].append((x - n, np.full(n, ACGT[two[0]])))
                big[ci]["plants"].append((x, np.full(n, ACGT[two[1]])))
                spans += [(x - n, x), (x, x + n)]
            else:                                    # two repeats of one array closer than W, the border in the gap between them
                g1, g2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
                n1, n2 = n, pick()[0]
                r = _repeat(rng, n1 + g1 + g2 + n2, p, sub)
                gap = ACGT[rng.integers(0, 4, size=g1 + g2)]
                r[n1:n1 + g1 + g2] = gap
                big[ci]["plants"].append((B - g1 - n1, r))
                spans += [(B - g1 - n1, B - g1), (B + g2, B + g2 + n2)]
            placed.append({"c": c, "kind": kind, "big": ci, "B": B, "spans": spans, "idx": len(placed)})

    letters = ACGT[:2] if (T, W) == (3, 64) else ACGT
    contigs = []
    for ci, ctg in enumerate(big):
        top = max([b for _, b in ctg["busy"]] + [0])
        ln = max(int(rng.integers(20_000, 26_000)), top + int(rng.integers(400, 1500)))
        if (T, W) == (3, 64) or T == 0:
            ln = top + int(rng.integers(400, 1500))  # (every base of these is low-complexity: the oracle's time goes with the length)
        s = letters[rng.integers(0, len(letters), size=ln)].copy()
        ctg["busy"] += [(0, 300), (ln - 300, ln)]
        for q in rng.integers(300, ln - 300, size=8):   # single IUPAC letters, none within W in front of a planted neighbourhood (see _check_planted)
            if free(ctg, q - 10, q + W + 10):
                s[q] = OTHER[int(rng.integers(0, len(OTHER)))]
        for pos, arr in ctg["plants"]:
            s[pos:pos + len(arr)] = arr
        if not wide or ci != 1:                      # (d) flush with the start
            n, p = pick()
            s[:n] = _repeat(rng, n, p, ci % 2 == 1)
            placed.append({"c": 0, "kind": "d", "big": ci, "B": 0, "spans": [(0, n)], "idx": len(placed)})
        if not wide or ci != 0:                      # (e) flush with the end
            n, p = pick()
            s[ln - n:] = _repeat(rng, n, p, ci % 2 == 0)
            if ci == 2 and W - n - n // 2 >= 3:
                # a non-base W - 1.5 n in front of it: n / 2 words from before it are still in the window when the array is found (the
                # stale-window quirk), and the interval is reported n / 2 further right: it ends beyond the contig
                s[ln - n - (W - n - n // 2) - 1] = ord("N")
            placed.append({"c": 0, "kind": "e", "big": ci, "B": ln, "spans": [(ln - n, ln)], "idx": len(placed)})
        contigs.append(s)
    for pl in placed:                                # lower case / bytes 0..3 over whole planted neighbourhoods
        if pl["c"] and pl["idx"] % 4 == 1:
            s = contigs[pl["big"]]
            lo, hi = pl["B"] - left, pl["B"] + right
            seg = s[lo:hi]
            up = np.isin(seg, ACGT)
            if pl["idx"] % 8 == 1 or not codes:
                seg[up] |= 0x20                      # acgt
            else:
                seg[up] = np.searchsorted(ACGT, seg[up]).astype(np.uint8)      # 0 1 2 3, which seq_nt4_table maps to themselves

    def tiny(n):
        """a whole array up to 66 bases; beyond, random letters around an array of 60 (the oracle's time on an array grows with the cube of its length)"""
        if n <= 66:
            return _repeat(rng, n, 1 + n % 2, False) if n else np.zeros(0, np.uint8)
        t = letters[rng.integers(0, len(letters), size=n)].copy()
        if not wide or n == W + 1:
            t[n - 62:n - 2] = _repeat(rng, 60, 1 + n % 2, False)
        return t
    small = letters[rng.integers(0, len(letters), size=700)].copy()           # shorter than the default chunk, with a repeat of its own
    small[300:380] = _repeat(rng, 80, 1, False)
    seqs, where = [], {}
    extras = [[tiny(0), tiny(1)], [tiny(2), tiny(W - 1)], [tiny(W), tiny(W + 1), tiny(13), small]]
    for ci, s in enumerate(contigs):
        where[ci] = len(seqs)
        seqs.append(s)
        if ci < 3:
            seqs += extras[ci]
    k = _Case()
    k.T, k.W = T, W
    k.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    k.placed = [dict(pl, ctg=where[pl["big"]]) for pl in placed]
    t0 = time.perf_counter()
    k.per_ctg = [[(int(r) >> 32, int(r) & 0xFFFFFFFF) for r in ob.sdust(s, T, W)] for s in k.seqs]
    k.oracle_s = time.perf_counter() - t0
    k.exp = [(ci, a, b) for ci, iv in enumerate(k.per_ctg) for a, b in iv]
    return k


def _check_planted(k, c):
    """the oracle reported something over every repeat planted for chunk size c (and the contig ends), and an interval over the border itself
    where a repeat straddles it"""
    if k.T > 100000:
        assert k.exp == []                           # (module docstring: no interval can exist at such a T)
        return
    kinds = set()
    for pl in k.placed:
        if pl["c"] not in (0, c):
            continue
        iv = k.per_ctg[pl["ctg"]]
        # (c) has non-bases less than W in front of its repeat: the window still holds the words from before them while the reference
        # already counts the window's start from behind them (the stale-window quirk), and the interval is reported up to W further right
        slack = k.W if pl["kind"] == "c" else 0
        for s, e in pl["spans"]:
            assert any(a < e + slack and b > s for a, b in iv), ("the oracle masks nothing over a planted repeat", k.T, k.W, pl)
        if pl["kind"] == "a":
            assert any(a < pl["B"] < b for a, b in iv), ("no interval over the border", k.T, k.W, pl)
        if pl["kind"] == "g":
            x = pl["spans"][0][1]
            assert any(a < x - 20 and b > x + 20 for a, b in iv), ("the two arrays are not one interval", k.T, k.W, pl)
        kinds.add(pl["kind"])
    assert kinds == {"a", "b1", "b2", "c", "d", "e", "f", "h"} | (set() if k.W > 257 else {"g"}), kinds


def _gpu(acc, seqs, T, W):
    asm = acc.asm_upload(seqs)
    try:
        return [(int(x["ctg"]), int(x["start"]), int(x["finish"])) for x in acc.sdust(asm, T, W)]
    finally:
        asm.close()


# ---- 1. oracle-exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W,chunk", [(T, W, ch) for T, W in PAIRS for ch in _chunks(W)])
def test_seams_vs_oracle(dacc, monkeypatch, T, W, chunk):
    k = _case_for(T, W, chunk)
    c = _chunk_value(chunk, W)
    _check_planted(k, c)
    if c <= max(W, 64):                              # the small decompositions: more than one workgroup's worth of chunks and lanes
        assert _n_chunks(k.seqs, c) > 64
    monkeypatch.setenv("CORNETTO_SDUST_CHUNK", chunk)
    got = _gpu(dacc, k.seqs, T, W)
    assert got == k.exp, (T, W, chunk, _first_diff(got, k.exp))


def _dense_blocks(rng, n, units, rep, gap):
    """n bases: one unit after the other repeated to `rep` bases, `gap` random bases between two"""
    s = ACGT[rng.integers(0, 4, size=n)].copy()
    for i, p in enumerate(range(gap, n - rep - gap, rep + gap)):
        s[p:p + rep] = np.resize(np.frombuffer(units[i % len(units)], dtype=np.uint8), rep)
    return s


# units whose 3-mers are pairwise different: arrays of two of them in one window add nothing to each other's score
DISJOINT = [b"A", b"C", b"G", b"T", b"AC", b"AG", b"AT", b"CG", b"CT", b"GT"]


@pytest.mark.parametrize("T,W,chunk,cap_env,rep,gap", [
    (1, 5, "520", None, 5, 7),          # sdust_kernel<64>: cap = max(16, 520 / 32) = 16
    (20, 67, "520", None, 16, 8),       # sdust_kernel<256>: 16 as well
    (40, 258, "2580", "3", 60, 300),    # sdust_kernel_g: CORNETTO_SDUST_CAP=3 in place of max(16, 2580 / 32) = 80 (module docstring)
])
def test_overflow_retry_vs_oracle(monkeypatch, T, W, chunk, cap_env, rep, gap):
    """a chunk with more intervals than a row of the per-chunk table holds: the kernel counts on, the host sizes the rows by the densest chunk
    and launches again (`cap = ovf`); nothing is truncated.  On a handle of its own: cap is raised to what the handle's workspace already holds."""
    import cornetto_amd
    c = int(chunk)
    cap = int(cap_env) if cap_env else max(16, c // 32)
    rng = np.random.default_rng(5 * W + T)
    seqs = [_dense_blocks(rng, 9 * c + 77, DISJOINT, rep, gap), _dense_blocks(rng, c - 3, DISJOINT[::-1], rep, gap), ACGT[rng.integers(0, 4, size=3 * c)].copy()]
    exp = [(ci, int(r) >> 32, int(r) & 0xFFFFFFFF) for ci, s in enumerate(seqs) for r in ob.sdust(s, T, W)]
    # intervals that begin inside one chunk are recorded by that chunk, except the first, which may have been begun by the chunk before
    densest = max(sum(1 for ci, a, _ in exp if ci == 0 and j * c <= a < (j + 1) * c) for j in range(10))
    assert densest - 1 > cap, (densest, cap)
    monkeypatch.setenv("CORNETTO_SDUST_CHUNK", chunk)
    if cap_env:
        monkeypatch.setenv("CORNETTO_SDUST_CAP", cap_env)
    a = cornetto_amd.Accel(0, dev=True)
    try:
        n0 = a.launch_count()
        got = _gpu(a, seqs, T, W)
        launches = a.launch_count() - n0
    finally:
        a.close()
    assert got == exp, (T, W, chunk, _first_diff(got, exp))
    assert launches == 2, launches                   # the first attempt overflowed, the second had room


# ---- 2. decomposition invariance -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rich(W):
    """repeat-rich contigs: a 171-base satellite monomer with 2 % divergence between copies (3 kb), a homopolymer of 5 kb, (GGAAT)n, (AT)n,
    runs of non-bases inside and beside the arrays, an array flush with each contig end"""
    rng = np.random.default_rng(9000 + W)
    a = ACGT[rng.integers(0, 4, size=13_000)].copy()
    mono = ACGT[rng.integers(0, 4, size=171)]
    sat = np.tile(mono, 18)
    pos = rng.choice(len(sat), size=len(sat) // 50, replace=False)
    sat[pos] = ACGT[rng.integers(0, 4, size=len(pos))]
    a[600:600 + len(sat)] = sat
    a[4200:9200] = ord("A")
    a[6400:6403] = ord("N")
    a[9900:11_900] = np.resize(np.frombuffer(b"GGAAT", dtype=np.uint8), 2000)
    a[11_900:11_940] = ord("N")
    a[12_400:] = np.resize(np.frombuffer(b"ttaggg", dtype=np.uint8), 600)
    b = ACGT[rng.integers(0, 4, size=3600)].copy()
    b[:500] = ord("T")
    b[1200:2400] = np.resize(np.frombuffer(b"AT", dtype=np.uint8), 1200)
    b[3100:] = ord("c")
    return [a, np.zeros(0, np.uint8), b, ACGT[rng.integers(0, 4, size=W + 1)].copy()]


_one_chunk = {}


@pytest.mark.parametrize("W,chunk", [(W, ch) for W in RICH_W for ch in _chunks(W)])
def test_decomposition_invariance(dacc, monkeypatch, W, chunk):
    """T = 20: see the module docstring (section 2) for what this does and does not show"""
    seqs = _rich(W)
    if W not in _one_chunk:
        monkeypatch.setenv("CORNETTO_SDUST_CHUNK", str(max(len(s) for s in seqs)))
        _one_chunk[W] = _gpu(dacc, seqs, 20, W)
    ref = _one_chunk[W]
    # canonical form: by (ctg, start), start < finish, no two intervals of a contig touching or overlapping
    assert len(ref) > 0 and all(a < b for _, a, b in ref)
    assert all(p[0] < q[0] or (p[0] == q[0] and p[2] < q[1]) for p, q in zip(ref, ref[1:]))
    monkeypatch.setenv("CORNETTO_SDUST_CHUNK", chunk)
    asm = dacc.asm_upload(seqs)
    try:
        first = [(int(x["ctg"]), int(x["start"]), int(x["finish"])) for x in dacc.sdust(asm, 20, W)]
        again = [(int(x["ctg"]), int(x["start"]), int(x["finish"])) for x in dacc.sdust(asm, 20, W)]     # the chunk table cached with the assembly
    finally:
        asm.close()
    assert first == ref, (W, chunk, _first_diff(first, ref))
    assert again == first, (W, chunk, _first_diff(again, first))


# ---- 3. product build, drop-ins, CLI ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", PAIRS)
def test_product_build_default_chunking(acc, T, W):
    """every contig of 84 kb is longer than one default chunk (32 W at most 32 832), and the default's borders carry the planted repeats"""
    k = _case_for(T, W, "0")
    _check_planted(k, _default_chunk(W))
    assert max(len(s) for s in k.seqs) > 32 * W
    got = _gpu(acc, k.seqs, T, W)
    assert got == k.exp, (T, W, _first_diff(got, k.exp))


@pytest.mark.parametrize("T,W", PAIRS)
def test_dropins_default_chunking(T, W):
    """cornetto_sdust() and cornetto_sdust_core(), contig by contig (lengths given: bytes 0..3 are part of the input)"""
    import cornetto_amd
    L = cornetto_amd.lib()
    L.cornetto_sdust.restype = C.POINTER(C.c_uint64)
    L.cornetto_sdust.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.cornetto_sdust_buf_init.restype = C.c_void_p
    L.cornetto_sdust_buf_init.argtypes = [C.c_void_p]
    L.cornetto_sdust_buf_destroy.argtypes = [C.c_void_p]
    L.cornetto_sdust_core.restype = C.POINTER(C.c_uint64)
    L.cornetto_sdust_core.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    k = _case_for(T, W, "0")
    buf = L.cornetto_sdust_buf_init(None)
    assert buf
    try:
        for ci, s in enumerate(k.seqs):
            exp = [a << 32 | b for a, b in k.per_ctg[ci]]
            cb = C.create_string_buffer(s.tobytes(), len(s) + 1)
            n = C.c_int()
            r = L.cornetto_sdust(None, C.cast(cb, C.c_void_p), len(s), T, W, C.byref(n))
            assert n.value >= 0 and r
            got = [int(r[i]) for i in range(n.value)]
            libc.free(C.cast(r, C.c_void_p))
            assert got == exp, ("cornetto_sdust", T, W, ci, len(s))
            r = L.cornetto_sdust_core(C.cast(cb, C.c_void_p), len(s), T, W, C.byref(n), buf)
            assert n.value >= 0 and r
            assert [int(r[i]) for i in range(n.value)] == exp, ("cornetto_sdust_core", T, W, ci, len(s))
    finally:
        L.cornetto_sdust_buf_destroy(buf)
    if (T, W) in ((80, 530), (25, 130), (4, 66)):    # one pair per kernel: the unmodified reference's own sdust() where it is built, as in test_fuzz_small.py
        if not os.path.exists(REFSO):
            pytest.skip("oracle/_ref/libcornetto_ref.so not built (the oracle comparison above ran)")
        ci = int(np.argmax([len(s) for s in k.seqs]))
        ref = ref_sdust(REFSO, [(k.seqs[ci], T, W)])[0]
        assert [int(x) for x in ref] == [a << 32 | b for a, b in k.per_ctg[ci]]


@pytest.mark.parametrize("T,W", [(80, 530), (25, 100)])
def test_cli_wide_windows(tmp_path, T, W):
    """`cornetto sdust -w W -t T` on a written FASTA (the letters-only form of the pair's assembly, 60 bases per line) against text formatted
    from the oracle, and against the unmodified reference binary's stdout where that is built"""
    import cornetto_amd
    k = _case_for(T, W, "0", False)
    _check_planted(k, _default_chunk(W))
    fa = tmp_path / "wide.fa"
    with open(fa, "wb") as f:
        for ci, s in enumerate(k.seqs):
            b = s.tobytes()
            f.write(b">ctg%d len=%d\n" % (ci, len(b)) + b"".join(b[i:i + 60] + b"\n" for i in range(0, len(b), 60)))
    exp = b"".join(fmt_sdust(b"ctg%d" % ci, np.array([a << 32 | b for a, b in iv], dtype=np.uint64)) for ci, iv in enumerate(k.per_ctg))
    args = ["sdust", "-w", str(W), "-t", str(T), str(fa)]
    p = subprocess.run([cornetto_amd.CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-300:]
    assert p.stdout == exp
    if os.path.exists(REFCLI):
        pr = subprocess.run([REFCLI] + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        assert (pr.returncode, pr.stdout) == (0, exp)


if __name__ == "__main__":      # the oracle's time per pair (no device needed): what the budget in the module docstring was measured with
    total = 0.0
    seen = set()
    for T, W in PAIRS:
        for ch in _chunks(W):
            k = _case_for(T, W, ch)
            c = _chunk_value(ch, W)
            _check_planted(k, c)
            if id(k) in seen:
                continue
            seen.add(id(k))
            print("T %7d W %4d chunk %5s: oracle %5.2f s, %d bases in %d contigs, %d intervals (%d beyond a contig's end), %d planted, %d chunks" % (
                T, W, ch, k.oracle_s, sum(map(len, k.seqs)), len(k.seqs), len(k.exp), sum(1 for ci, _, b in k.exp if b > len(k.seqs[ci])),
                len(k.placed), _n_chunks(k.seqs, c)), flush=True)
            total += k.oracle_s
    print("total %.1f s" % total)
    sys.exit(0)
