"""GPU: tf_scan (csrc/telo.hip) at its own seams, every result compared with the oracle (tests/telofind_cases.py).

The other tests of this stage place runs at random: a run meets a tile seam about once per motif at an arbitrary phase, the row limit is
either far away or far exceeded, and the marks are only seen through `car` of windows over a positive threshold.  Here, for every template
of the kernel (H = 7, 15, 31 at their longest motifs without a wildcard, and the byte-wise form), every split of a copy lies over a segment
seam, over a tile seam inside a workgroup and over one between two workgroups, with one to three copies, both strands, decoys one letter
off, lower case and copies flush with the contig ends; one tile holds exactly 32 and exactly 33 entries in one of its lists; a tile holds as
many entries as a tile can; and the mark bitmap is compared word by word, the bits behind every contig's end included.  Exact integer and
bit comparisons throughout.  tests/test_telofind_cases_host.py checks without a device that the cases are what they are named for."""
import numpy as np
import pytest

import cornetto_amd
import selftest_bind as sb
import telofind_cases as tc
from test_gpu_telowin import names_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def ident(m):
    return "k%d-%s" % (len(m), m[:12].decode())


def place(seqs, ctg, pos):
    """where position pos of contig ctg lies for tf_scan: tile, thread, and the nearest seam with its kind"""
    first = int(sum(-(-len(s) // tc.TILE) for s in seqs[:ctg]))
    g = first + pos // tc.TILE
    m = (pos + tc.SEG // 2) // tc.SEG * tc.SEG
    kind = "segment" if m % tc.TILE else "group" if (first + m // tc.TILE) % tc.NT == 0 else "tile"
    return "contig %d (length %d) position %d = global tile %d (tile %d of workgroup %d), thread %d, bit %d; nearest seam %d (%s, %+d)" % (
        ctg, len(seqs[ctg]), pos, g, g % tc.NT, g // tc.NT, 1 + pos % tc.TILE // tc.SEG, pos % tc.SEG, m, kind, pos - m)


def same_rows(got, exp, seqs, what):
    """equal rows; the first difference by contig, position and seam"""
    assert got.dtype == exp.dtype, (got.dtype, exp.dtype)
    if len(got) == len(exp) and np.array_equal(got, exp):
        return
    i = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    g, e = got[i] if i < len(got) else None, exp[i] if i < len(exp) else None
    r = e if e is not None else g
    assert False, "%s: %d rows against %d expected; first difference at row %d: got %s, expected %s; %s" % (
        what, len(got), len(exp), i, g, e, place(seqs, int(r["ctg"]), int(r["start"])))


def same_words(got, exp, seqs, what):
    """equal mark words; the first difference by contig, position and seam, the differing bits named"""
    assert got.dtype == exp.dtype == np.uint64 and len(got) == len(exp), (got.dtype, len(got), len(exp))
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return
    w0 = np.concatenate([[0], np.cumsum([-(-len(s) // 64) for s in seqs])])
    i = int(bad[0])
    ctg = int(np.searchsorted(w0, i, side="right")) - 1
    x = int(got[i]) ^ int(exp[i])
    pos = 64 * (i - int(w0[ctg])) + (x & -x).bit_length() - 1
    assert False, "%s: %d of %d words differ; first: word %d got %016x expected %016x (xor %016x); %s%s" % (
        what, len(bad), len(exp), i, int(got[i]), int(exp[i]), x, place(seqs, ctg, pos), " — behind the contig's end" if pos >= len(seqs[ctg]) else "")


def run_all(acc, dacc, seqs, motif, what):
    """the four comparisons of one case on one upload per handle -> (launch names of telofind, of telo_scan, of the marks)"""
    rows, words, wins = tc.expected(seqs, motif)
    asm = acc.asm_upload(seqs)
    try:
        same_rows(acc.telofind(asm, motif), rows, seqs, "%s: telofind" % what)
        nm_find = names_of(acc)
        for again in ("", " again"):
            hits, w = acc.telo_scan(asm, motif, 0.0)
            nm_scan = names_of(acc)
            same_rows(hits, rows, seqs, "%s: hits of telo_scan%s" % (what, again))
            same_rows(w, wins, seqs, "%s: windows of telo_scan%s at 0" % (what, again))
    finally:
        asm.close()
    dasm = dacc.asm_upload(seqs)
    try:
        same_words(sb.telo_marks(dacc, dasm, motif, len(words)), words, seqs, "%s: marks" % what)
        nm_marks = names_of(dacc)
    finally:
        dasm.close()
    return nm_find, nm_scan, nm_marks


@pytest.mark.parametrize("motif", tc.MOTIFS, ids=ident)
def test_every_split_over_every_seam(acc, dacc, motif):
    """seam_case: rows of telofind, hits and every window of the fused scan, the same again on the resident assembly, and the mark words.  A
    motif without a border takes the rows and a gather (no tile holds more than 6 entries) and tf_scan's own marks in its count-only mode;
    one with a border or beyond 32 letters takes every match, the greedy rule, and the marks of the runs."""
    case = tc.seam_case(motif)
    nm_find, nm_scan, nm_marks = run_all(acc, dacc, case.seqs, motif, ident(motif))
    if motif in tc.UNBORDERED:
        assert nm_find.count("tf_scan") == 1 and "tf_gather" in nm_find and "tf_greedy" not in nm_find, nm_find
        assert nm_scan.count("tf_scan") == 1 and "tf_gather" in nm_scan and "tw_scan" in nm_scan and "tw_fill" not in nm_scan, nm_scan
        assert nm_marks.count("tf_scan") == 1 and "tf_gather" not in nm_marks and "tw_fill" not in nm_marks, nm_marks
    else:
        assert nm_find.count("tf_scan") == 2 and "tf_greedy" in nm_find and "tf_gather" not in nm_find, nm_find
        assert "tw_fill" in nm_scan and "tw_fill" in nm_marks, (nm_scan, nm_marks)


@pytest.mark.parametrize("n_fwd,n_rev,where,counts", tc.ROW_CASES)
def test_the_row_limit(acc, dacc, n_fwd, n_rev, where, counts):
    """row_case: exactly 32 entries in a list keep the single pass and the gather, 33 in any one list take the second pass instead"""
    case = tc.row_case(n_fwd, n_rev, where)
    nm_find, nm_scan, nm_marks = run_all(acc, dacc, case.seqs, tc.ROW_MOTIF, "%d/%d %s" % (n_fwd, n_rev, where))
    for nm in (nm_find, nm_scan):
        if max(counts) <= tc.ROW:
            assert nm.count("tf_scan") == 1 and nm.count("tf_gather") == 1, nm
        else:
            assert nm.count("tf_scan") == 2 and "tf_gather" not in nm, nm
    assert "tw_scan" in nm_scan and "tw_fill" not in nm_scan, nm_scan
    assert nm_marks.count("tf_scan") == 1, nm_marks


def test_the_densest_tile(acc, dacc):
    """dense_case: 8128 entries in each of the four lists of a tile (the 16-bit counters of the packed scan, two per half), and 16256 matches in
    list 0 and in list 2"""
    (gc, m1), (poly, m2) = tc.dense_case()
    nm_find, nm_scan, _ = run_all(acc, dacc, gc, m1, "G over GC")
    assert nm_find.count("tf_scan") == 2 and "tf_gather" not in nm_find and nm_scan.count("tf_scan") == 2, (nm_find, nm_scan)
    nm_find, _, nm_marks = run_all(acc, dacc, poly, m2, "AAAA over poly-A and poly-T")
    assert "tf_greedy" in nm_find and "tw_fill" in nm_marks, (nm_find, nm_marks)
