"""The planted inputs of tests/test_gpu_sdust_sift.py, checked without a device: every kind of tests/sift_cases.py is present and masked by the
oracle for every pair and chunk-size set, the pairs that cannot mask anything mask nothing, and the row-capacity cases hold exactly the rows
they are named for.  Keeps the GPU module from silently losing its cases."""
import numpy as np
import pytest

import sift_cases as sc


@pytest.mark.parametrize("T,W", sc.PAIRS + sc.EMPTY)
def test_default_chunk_cases(T, W):
    k = sc.case(T, W)
    sc.check(k)
    assert k.cvals == (sc.CHUNK,) and len(k.placed) == len(sc.kinds_for(sc.CHUNK)) + len(sc.ONCE_KINDS) + (sc.t_eff(T, W) > 20)
    assert ((T, W) in sc.EMPTY) == (k.exp == [])
    # more than one wave's worth of chunks, contigs of one chunk and of several, walked chunks beside chunks of plain letters
    assert sc.n_chunks(k.seqs) > 64
    dirty = [ci for ci, s in enumerate(k.seqs) if not np.isin(s & 0xDF, sc.ACGT).all()]
    assert dirty and len(dirty) < len(k.seqs) // 2


@pytest.mark.parametrize("T,W", sc.RT_PAIRS)
def test_run_time_chunk_cases(T, W):
    k = sc.case(T, W, sc.RT_CHUNKS)
    sc.check(k)
    assert len(k.placed) == sum(len(sc.kinds_for(c)) for c in sc.RT_CHUNKS) + len(sc.ONCE_KINDS) + (sc.t_eff(T, W) > 20)
    for c in sc.RT_CHUNKS:                                # every border lies where it was planted for: a multiple of its chunk size
        assert all(pl["B"] % c == 0 and pl["B"] >= c for pl in k.placed if pl["c"] == c)
        assert sc.n_chunks(k.seqs, c) > 64


def test_pairs_are_the_ones_the_kernel_takes():
    for T, W in sc.PAIRS + sc.EMPTY:
        assert W <= 66 and 5 <= T <= 100000               # sd_sift's range (sdust_asm_impl)
    assert sc.CAP_ROWS == 56


def test_twin_case():
    k = sc.twin()
    assert 4_400_000 < sum(map(len, k.seqs)) < 4_600_000 and sc.n_chunks(k.seqs) > 2500
    assert {pl["kind"] for pl in k.placed} >= {"a", "b1", "b2", "f", "g", "h", "r1", "c0", "c1"}
    assert all(pl["B"] % (50 * sc.CHUNK) == 0 for pl in k.placed)


def test_capacity_cases():
    d = sc.cap_dense()
    assert max(sc.rows_per_chunk(d).values()) > sc.CAP_ROWS
    for rows in (56, 57):
        k = sc.cap_exact(rows)
        got = sc.rows_per_chunk(k)
        assert got[sc.CAP_AT] == rows
        assert max(v for kk, v in got.items() if kk != sc.CAP_AT) < rows
        assert all(np.isin(s, sc.ACGT).all() for s in k.seqs)         # no walked chunk: the rows are the recording rule's
        # the next chunk's first start is exactly this chunk's end - W
        assert ((sc.CAP_AT[1] + 1) * sc.CHUNK - k.W) in [a for a, _ in k.per_ctg[sc.CAP_AT[0]]]
        # the intervals of the designated chunk lie apart: one row each, none shared with a neighbour
        mine = [(a, b) for a, b in k.per_ctg[0] if (a + k.W) // sc.CHUNK == sc.CAP_AT[1]]
        assert len(mine) == rows and all(q[0] > p[1] + 1 for p, q in zip(mine, mine[1:]))
