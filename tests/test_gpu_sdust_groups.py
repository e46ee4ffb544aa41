"""sd_sift's chunk groups (cornetto_amd/csrc/sdust_sift.hpp): a counter request hands out SIFT_GROUP consecutive chunks, and inside a group a
chunk of plain letters takes the seam tile over from the chunk before instead of redoing it.  Every comparison is exact equality of
(ctg, start, finish) with the CPU oracle, on the assemblies of tests/group_cases.py (what is planted where: its docstring;
tests/test_sdust_groups_host.py checks the cases themselves without a device) and on the planted assemblies of tests/sift_cases.py.

  a  the product library, call after call on one resident assembly (the first call; two with the `order` table and the fused tail; another
     pair in between), the group cases and the planted pairs of sift_cases
  b  the development library: the literal-size build and, with CORNETTO_SIFT_GENERIC=1, the run-time-size build
  c  one wave and three waves through every chunk; the product with the smallest share it takes
  d  the counting build: the seams it carried are the closed form of the group size it reports and the contig layout; with bytes planted that
     are no letters, fewer by exactly the seams those bytes take away
The group size is read from the counting build, and the cases are built for it.
"""
import numpy as np
import pytest

import group_cases as gc
import sift_cases as sc
from sift_cases import _first_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    import cornetto_amd
    a = cornetto_amd.Accel(0)
    assert a.lib_path == cornetto_amd.LIB_PATH
    yield a
    a.close()


@pytest.fixture(scope="module")
def G(acc):
    """the group size of the library under test, as its counting build reports it"""
    rng = np.random.default_rng(5)
    asm = acc.asm_upload([sc.ACGT[rng.integers(0, 4, size=2 * gc.CHUNK)].copy()])
    try:
        st = acc.sdust_stats(asm, 20, 64)
    finally:
        asm.close()
    assert st["kernel"] == "sd_sift" and st["chunks"] == 2, st
    g = st["chunks_per_group"]
    assert g >= 2 and g & (g - 1) == 0, st
    assert st["seams_carried"] == 1, st
    return g


def _t(iv):
    return [(int(x["ctg"]), int(x["start"]), int(x["finish"])) for x in iv]


def _no_switches(monkeypatch):
    for name in ("CORNETTO_SDUST_CHUNK", "CORNETTO_SIFT_GENERIC", "CORNETTO_SIFT_BLOCKS", "CORNETTO_SDUST_SIFT", "CORNETTO_SIFT_DP", "CORNETTO_SIFT_L2SKIP",
                 "CORNETTO_SDUST_CAP", "CORNETTO_SIFT_ABL"):
        monkeypatch.delenv(name, raising=False)


# ---- a. the product build, call after call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", gc.PAIRS)
def test_call_sequence(acc, G, T, W):
    """contig lengths around one chunk, two chunks, a group and a group and a chunk; runs of short contigs; features against the last 128 bases
    of a chunk at carried and at redone seams; a byte that is no letter in the middle, the last 128 and the first base of a group's second chunk"""
    k = gc.assembly(T, W, G)
    gc.check(k)
    T2, W2 = (12, 34) if (T, W) == (20, 64) else (20, 64)
    exp2 = gc.other_exp(T, W, G, T2, W2)
    asm = acc.asm_upload(k.seqs)
    try:
        calls = [_t(acc.sdust(asm, T, W)) for _ in range(3)]
        other = _t(acc.sdust(asm, T2, W2))
        after = _t(acc.sdust(asm, T, W))
    finally:
        asm.close()
    for i, got in enumerate(calls):
        assert got == k.exp, (T, W, G, "call %d" % i, _first_diff(got, k.exp))
    assert other == exp2, (T, W, G, "then", T2, W2, _first_diff(other, exp2))
    assert after == k.exp, (T, W, G, "after", T2, W2, _first_diff(after, k.exp))


@pytest.mark.parametrize("T,W", sc.PAIRS + sc.EMPTY)
def test_planted_pairs(acc, G, T, W):
    """the planted borders of sift_cases, which the groups now run through in twos, fours or eights: a first call and one with `order`"""
    k = sc.case(T, W)
    asm = acc.asm_upload(k.seqs)
    try:
        first, again = _t(acc.sdust(asm, T, W)), _t(acc.sdust(asm, T, W))
    finally:
        asm.close()
    assert first == k.exp, (T, W, _first_diff(first, k.exp))
    assert again == k.exp, (T, W, "second call", _first_diff(again, k.exp))


# ---- b. both development builds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", ["0", "1"])
@pytest.mark.parametrize("T,W", gc.PAIRS)
def test_both_development_builds(dacc, monkeypatch, G, T, W, generic):
    _no_switches(monkeypatch)
    if generic == "1":
        monkeypatch.setenv("CORNETTO_SIFT_GENERIC", "1")
    k = gc.assembly(T, W, G)
    asm = dacc.asm_upload(k.seqs)
    try:
        first, again = _t(dacc.sdust(asm, T, W)), _t(dacc.sdust(asm, T, W))
    finally:
        asm.close()
    assert first == k.exp, (T, W, generic, _first_diff(first, k.exp))
    assert again == k.exp, (T, W, generic, "second call", _first_diff(again, k.exp))


# ---- c. wave counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("T,W", gc.PAIRS)
def test_few_waves_through_every_group(dacc, monkeypatch, G, T, W, blocks):
    """CORNETTO_SIFT_BLOCKS=1: ONE wave works through every group in the order of the 64 counters — group g + 64 behind group g, whose last
    chunk it must not take a seam from — 3: three waves"""
    _no_switches(monkeypatch)
    monkeypatch.setenv("CORNETTO_SIFT_BLOCKS", blocks)
    for k in (gc.assembly(T, W, G), sc.case(T, W)):
        asm = dacc.asm_upload(k.seqs)
        try:
            first, again = _t(dacc.sdust(asm, T, W)), _t(dacc.sdust(asm, T, W))
        finally:
            asm.close()
        assert first == k.exp, (T, W, blocks, _first_diff(first, k.exp))
        assert again == k.exp, (T, W, blocks, "second call", _first_diff(again, k.exp))


def test_product_with_the_smallest_share(G):
    import cornetto_amd
    k = gc.assembly(20, 64, G)
    a = cornetto_amd.Accel(0)
    try:
        a.set_share(10)
        try:
            asm = a.asm_upload(k.seqs)
            try:
                first, again = _t(a.sdust(asm, k.T, k.W)), _t(a.sdust(asm, k.T, k.W))
            finally:
                asm.close()
        finally:
            a.set_share(100)
    finally:
        a.close()
    assert first == k.exp, _first_diff(first, k.exp)
    assert again == k.exp, ("second call", _first_diff(again, k.exp))


# ---- d. the counting build -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", gc.PAIRS)
def test_counted_seams(acc, G, T, W):
    """The counting pass is the FIRST call for its assembly: no `order` table yet, so chunk i of the table is position i of the hand-out order.
    Letters only: every chunk that is neither the first of its contig nor the first of its group takes its seam over.  With the three bytes:
    fewer by the seams gc.lost_seams() names."""
    letters, k = gc.assembly(T, W, G, dirty=False), gc.assembly(T, W, G)
    out = []
    for case in (letters, k):
        asm = acc.asm_upload(case.seqs)
        try:
            st, iv = acc.sdust_stats(asm, T, W, intervals=True)
        finally:
            asm.close()
        print("sd_sift stats", (T, W, G), st)
        assert st["kernel"] == "sd_sift" and st["chunks_per_group"] == G and st["chunks"] == len(gc.chunk_table(case.seqs)), st
        got = _t(iv)
        assert got == case.exp, (T, W, G, "counting build", _first_diff(got, case.exp))
        out.append(st)
    assert out[0]["base_by_base_steps_of_chunks_with_other_bytes"] == 0 and out[1]["base_by_base_steps_of_chunks_with_other_bytes"] > 0, out
    assert out[0]["seams_carried"] == gc.closed_form(letters.seqs, G), out[0]
    assert out[1]["seams_carried"] == gc.closed_form(k.seqs, G) - len(gc.lost_seams(k)) == len(gc.carried(k.seqs, G)), out[1]
