"""The planted inputs of tests/test_gpu_telofind_seams.py, checked without a device: for every motif of tests/telofind_cases.py the oracle
reports exactly the planted runs and no decoy, every split lies over every kind of seam, the row cases hold exactly the counts they are named
for and the dense cases reach a tile's maximum.  Keeps the GPU module from silently losing its cases: nothing here is skipped or filtered."""
import numpy as np
import pytest

import telofind_cases as tc


def ident(m):
    return "k%d-%s" % (len(m), m[:12].decode())


@pytest.mark.parametrize("motif", tc.MOTIFS, ids=ident)
def test_seam_case(motif):
    k = len(motif)
    case = tc.seam_case(motif)
    rows, words, wins = tc.expected(case.seqs, motif)
    assert len({len(s) for s in case.seqs}) == 1 and len(case.seqs[0]) == 4 * tc.TILE + 200
    assert list(case.first_tile) == [5 * i for i in range(len(case.seqs) + 1)]

    # the oracle's runs are the planted ones, each as it stands on its own, and no decoy is reported
    exp = tc.planted(case)
    assert len(rows) == len(exp) and np.array_equal(rows, exp)
    decoys = tc.decoy_spans(case)
    by_ctg = {}
    for c, a, b in decoys:
        by_ctg.setdefault(c, []).append((a, b))
    if k > 1:
        # beside one seam of every contig (both decoys wherever three copies of the motif leave room), and over tile and group seams as well
        per = [len(by_ctg.get(c, ())) for c in range(len(case.seqs))]
        assert min(per) >= 1 and (k > 16 or min(per) >= 2) and sum(x >= 2 for x in per) >= 0.95 * len(per), per
        over = tc.decoy_census(case)
        assert over["segment"] and over["tile"] and over["group"], over
    for r in rows:
        assert all(int(r["end"]) <= a or b <= int(r["start"]) for a, b in by_ctg.get(int(r["ctg"]), ()))
    # a plant at the contig's first base and one flush with its end, both units, lower case in some contigs and not in others
    for strand in {0, 1} if k > 1 else {0}:
        mine = rows[rows["strand"] == strand]
        assert (mine["start"] == 0).any() and (mine["end"] == 4 * tc.TILE + 200).any()
    lower = [bool((s >= ord("a")).any()) for s in case.seqs]
    assert any(lower) and not all(lower)

    # every split over every kind of seam
    got = tc.census(case)
    # (k > 32: the listed d; a stretch is cut where its occurrences of the motif are cut)
    need = set(range(1, k)) if k <= tc.MAX_MOTIF else {d for d in tc.split_list(motif) if 0 < d < k}
    for kind in ("segment", "tile", "group"):
        assert need <= got[kind], (kind, sorted(need - got[kind]))

    # rows mode stays in force (a motif without a border): no tile comes near the row limit by accident
    if not tc.uses_stretches(motif) and k <= tc.MAX_MOTIF:
        assert max(max(v) for v in tc.list_counts(case, rows).values()) <= 6
    # what the marks and the windows are compared by
    assert len(words) == tc.n_words(case.seqs) and int(sum(bin(int(w)).count("1") for w in words[words != 0])) > 0
    assert len(wins) == len(case.seqs) * 323 and int(wins["car"].sum()) > 0


def test_sizes():
    """12 to 198 contigs per motif without a border, the largest under 13 MB"""
    n = [tc.n_contigs(m) for m in tc.UNBORDERED]
    assert all(len(tc.seam_case(m).seqs) == tc.n_contigs(m) for m in tc.UNBORDERED[:5])
    assert min(n) == 12 and max(n) == 198 and max(n) * tc.CTG_LEN < 13_000_000


@pytest.mark.parametrize("n_fwd,n_rev,where,counts", tc.ROW_CASES)
def test_row_case(n_fwd, n_rev, where, counts):
    case = tc.row_case(n_fwd, n_rev, where)
    rows, _, _ = tc.expected(case.seqs, tc.ROW_MOTIF)
    exp = tc.planted(case)
    assert len(rows) == len(exp) and np.array_equal(rows, exp)
    assert [len(s) for s in case.seqs] == [3 * tc.TILE] * 3 and list(case.first_tile) == [0, 3, 6, 9]
    got = tc.list_counts(case, rows)
    at = tc.row_at(where)
    assert tuple(got[at]) == counts
    assert len(got) == 9 and max(max(v) for kk, v in got.items() if kk != at) < tc.ROW
    if where == "flush":
        assert ((rows["ctg"] == at[0]) & (rows["end"] == (at[1] + 1) * tc.TILE) & (rows["strand"] == 0)).sum() == 1
    # isolated copies at least 7 bases apart (the two-copy run of tail_next / head_prev aside)
    for c in range(3):
        mine = np.sort(rows[rows["ctg"] == c], order="start")
        assert (mine["start"][1:] - mine["end"][:-1] >= 7).all()
        assert ((mine["end"] - mine["start"]) == 6).sum() == len(mine) - (c == at[0] and where in ("tail_next", "head_prev"))


def test_dense_case():
    (gc, m1), (poly, m2) = tc.dense_case()
    assert m1 == b"G" and not tc.border(m1) and m2 == b"AAAA" and tc.border(m2)
    assert [len(s) for s in gc] == [2 * tc.TILE + 3] and [len(s) for s in poly] == [2 * tc.TILE + 3] * 2
    rows, _, _ = tc.expected(gc, m1)
    counts = tc.list_counts(tc.Case(m1, gc, [[]]), rows)
    assert counts[(0, 0)] == [tc.TILE // 2] * 4 == [8128] * 4 and counts[(0, 1)] == [8128] * 4 and sorted(counts[(0, 2)]) == [1, 1, 2, 2]
    assert 8128 < 1 << 15
    mc = tc.match_counts(poly, m2)
    assert mc[(0, 0)] == [tc.TILE, 0] == [16256, 0] and mc[(1, 0)] == [0, 16256] and mc[(0, 1)] == [16256, 0] and mc[(1, 1)] == [0, 16256]
    assert 16256 < 1 << 15
    # the greedy rule: one run over the whole of poly-A, cut to a multiple of 4
    prow, _, _ = tc.expected(poly, m2)
    assert [tuple(map(int, r)) for r in prow] == [(0, 0, 0, 2 * tc.TILE), (1, 1, 0, 2 * tc.TILE)]


def test_motif_claims():
    for m in tc.UNBORDERED:
        assert not tc.border(m) and not tc.border(tc.revcomp(m)) and tc.period(m) == len(m)
    assert [tc.template(m) for m in tc.UNBORDERED] == [7] * 8 + [15] * 2 + [31] * 3
    for m in tc.BORDERED:
        assert tc.border(m) and 1 <= tc.period(m) < len(m) <= tc.MAX_MOTIF
    assert [tc.template(m) for m in tc.BORDERED] == [7, 7, 7, 7, 31]
    assert all(tc.template(m) == -1 for m in tc.LONG)
    assert (tc.SEG, tc.TILE, tc.NT, tc.ROW, tc.MAX_MOTIF) == (64, 254 * 64, 4, 32, 32)
    # runs_of restates the oracle's rule
    import oracle_bind as ob
    for text, pat in ((b"ACACACA", b"ACACA"), (b"AAAAAAAAA", b"AAAA"), (b"TTAGGGTTAGGGTTAGGG", b"TTAGGGTT"), (b"GGTTAGGGTTAGGGCC", b"TTAGGG")):
        oh = ob.telofind(text, pat)
        assert [(int(h["start"]), int(h["end"])) for h in oh[oh["strand"] == 0]] == tc.runs_of(text, pat)
