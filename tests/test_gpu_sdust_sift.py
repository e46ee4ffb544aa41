"""sd_sift (cornetto_amd/csrc/sdust_sift.hpp) at its own seams, in the instantiation the product runs — every comparison is exact equality of
(ctg, start, finish) with the CPU oracle, on the planted assemblies of tests/sift_cases.py (what is planted where: its docstring;
tests/test_sift_cases_host.py checks the cases themselves without a device).

  a  the product library at its default decomposition (sd_sift<false, SIFT_CAP_DEFAULT>): every pair, call after call on one resident
     assembly, another pair in between; one pass of the counting build (sd_sift<true>) shows that the input reached the stages it was
     built for, and its intervals are compared as well
  b  the development library on the same assemblies: the literal-size build and, with CORNETTO_SIFT_GENERIC=1, the run-time-size build
     at the same decomposition
  c  the run-time-size build at its own chunk sizes, the assemblies planted for each of them
  d  one wave (and three) through every chunk; the product with the smallest share it takes
  e  a chunk with exactly as many rows as the first attempt holds, with one more, with many more
"""
import numpy as np
import pytest

import sift_cases as sc
from sift_cases import _first_diff

pytestmark = pytest.mark.gpu

ALL = sc.PAIRS + sc.EMPTY
ONE_WAVE_PAIRS = [(20, 64), (5, 7), (20, 66), (319, 66)]


@pytest.fixture(scope="module")
def acc():
    import cornetto_amd
    a = cornetto_amd.Accel(0)
    assert a.lib_path == cornetto_amd.LIB_PATH
    yield a
    a.close()


def _t(iv):
    return [(int(x["ctg"]), int(x["start"]), int(x["finish"])) for x in iv]


def _no_switches(monkeypatch):
    for name in ("CORNETTO_SDUST_CHUNK", "CORNETTO_SIFT_GENERIC", "CORNETTO_SIFT_BLOCKS", "CORNETTO_SDUST_SIFT", "CORNETTO_SIFT_DP", "CORNETTO_SIFT_L2SKIP",
                 "CORNETTO_SDUST_CAP", "CORNETTO_SIFT_ABL"):
        monkeypatch.delenv(name, raising=False)


# ---- a. the product build, default chunking ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", ALL)
def test_product_default_chunking(acc, T, W):
    """three calls on one resident assembly (the first; the one with the `order` table and the fused tail; one more), another pair (the walk
    table is keyed by the decomposition only, the row estimate by (T, W) as well), the first pair again"""
    k = sc.case(T, W)
    sc.check(k)
    T2, W2 = (12, 34) if (T, W) == (20, 64) else (20, 64)
    exp2 = sc.other_exp(T, W, T2, W2)
    asm = acc.asm_upload(k.seqs)
    try:
        calls = [_t(acc.sdust(asm, T, W)) for _ in range(3)]
        st, civ = acc.sdust_stats(asm, T, W, intervals=True)
        print("sd_sift stats", (T, W), st)
        assert st is not None and st["kernel"] == "sd_sift", st
        # (if SIFT_CHUNK_DEFAULT ever changes this fails: the borders are planted for 1792)
        assert st["chunks"] == sum((len(s) + 1791) // 1792 for s in k.seqs) == sc.n_chunks(k.seqs), st
        assert st["base_by_base_steps_of_chunks_with_other_bytes"] > 0, st
        if (T, W) in sc.PAIRS:
            assert st["dp_tiles"] > 0, st
            assert st["resolve_steps"] > 0 and st["resolve_window_reads"] > 0, st
            gaps = st["window_reads_behind_a_gap_of"]
            # (W = 4: the window holds one word in front of the last, so a position is sifted exactly when its word equals the one before — a
            # homopolymer.  Sifted i and i + 2 around an unsifted i + 1 would need XXX, XXY, XYZ with XYZ = XXY, that is Y = X: no gap of 2 exists)
            # T = 319, W = 66: only a window of 64 equal words masks, a position is sifted only with 32 equal words in front of it (a homopolymer), and
            # behind b >= 3 broken words the partial sums of L1 refuse the next m positions until m (10 (63 - b) - 319) > 319 b: m >= 4, so the
            # shortest gap is 7
            assert gaps["2"] > 0 or W == 4 or T == 319, st
            assert gaps["3-4"] > 0 or T == 319, st
            assert gaps["5-8"] > 0, st
        for i, got in enumerate(calls):
            assert got == k.exp, (T, W, "call %d" % i, _first_diff(got, k.exp))
        got = _t(civ)
        assert got == k.exp, (T, W, "counting build", _first_diff(got, k.exp))
        got = _t(acc.sdust(asm, T2, W2))
        assert got == exp2, (T, W, "then", T2, W2, _first_diff(got, exp2))
        got = _t(acc.sdust(asm, T, W))
        assert got == k.exp, (T, W, "after", T2, W2, _first_diff(got, k.exp))
    finally:
        asm.close()


def test_letters_only_takes_no_base_by_base_step(acc):
    rng = np.random.default_rng(8)
    seqs = [sc.ACGT[rng.integers(0, 4, size=n)].copy() for n in (5000, 300)]
    seqs[0][2000:2400] = ord("a")
    asm = acc.asm_upload(seqs)
    try:
        st = acc.sdust_stats(asm, 20, 64)
    finally:
        asm.close()
    assert st["kernel"] == "sd_sift" and st["chunks"] == 4 and st["dp_tiles"] > 0, st
    assert st["base_by_base_steps_of_chunks_with_other_bytes"] == 0, st


# ---- b. both instantiations at one decomposition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", ["0", "1"])
@pytest.mark.parametrize("T,W", ALL)
def test_both_instantiations_default_chunking(dacc, monkeypatch, T, W, generic):
    """the development build without switches runs sd_sift<false, SIFT_CAP_DEFAULT> as the product does; CORNETTO_SIFT_GENERIC=1 runs
    sd_sift<false> on the same chunks.  Both equal the oracle, and so each other."""
    import cornetto_amd
    assert dacc.lib_path == cornetto_amd.DEV_LIB_PATH
    _no_switches(monkeypatch)
    if generic == "1":
        monkeypatch.setenv("CORNETTO_SIFT_GENERIC", "1")
    k = sc.case(T, W)
    asm = dacc.asm_upload(k.seqs)
    try:
        first, again = _t(dacc.sdust(asm, T, W)), _t(dacc.sdust(asm, T, W))
    finally:
        asm.close()
    assert first == k.exp, (T, W, generic, _first_diff(first, k.exp))
    assert again == k.exp, (T, W, generic, "second call", _first_diff(again, k.exp))


# ---- c. the run-time-size build at its own borders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [str(c) for c in sc.RT_CHUNKS])
@pytest.mark.parametrize("T,W", sc.RT_PAIRS)
def test_run_time_size_build_at_its_borders(dacc, monkeypatch, T, W, chunk):
    """256: the smallest size the sift stages take; 1920: a region of exactly two staging rounds; 1984: 64 bases in a third round, the path
    with its own loads; 3968: the largest, whose row extraction takes three rounds of 64 dwords with a carry between them"""
    k = sc.case(T, W, sc.RT_CHUNKS)
    sc.check(k)
    _no_switches(monkeypatch)
    monkeypatch.setenv("CORNETTO_SDUST_CHUNK", chunk)
    asm = dacc.asm_upload(k.seqs)
    try:
        first, again = _t(dacc.sdust(asm, T, W)), _t(dacc.sdust(asm, T, W))
        st = dacc.sdust_stats(asm, T, W)
    finally:
        asm.close()
    assert first == k.exp, (T, W, chunk, _first_diff(first, k.exp))
    assert again == k.exp, (T, W, chunk, "second call", _first_diff(again, k.exp))
    assert st["kernel"] == "sd_sift" and st["chunks"] == sc.n_chunks(k.seqs, int(chunk)), st


@pytest.mark.parametrize("chunk", ["192", "4032"])
def test_sizes_outside_the_sift_range_fall_back(dacc, monkeypatch, chunk):
    """below 256 and above 3968 bases the host takes the per-lane kernel by itself: the same intervals"""
    T, W = 20, 64
    k = sc.case(T, W, sc.RT_CHUNKS)
    _no_switches(monkeypatch)
    monkeypatch.setenv("CORNETTO_SDUST_CHUNK", chunk)
    asm = dacc.asm_upload(k.seqs)
    try:
        got = _t(dacc.sdust(asm, T, W))
        st = dacc.sdust_stats(asm, T, W)
    finally:
        asm.close()
    assert got == k.exp, (chunk, _first_diff(got, k.exp))
    assert st is None or st.get("kernel") != "sd_sift", st


# ---- d. one wave takes every chunk -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("T,W", ONE_WAVE_PAIRS)
def test_one_wave_through_every_chunk(dacc, monkeypatch, T, W, blocks):
    """CORNETTO_SIFT_BLOCKS=1: ONE wave works through clean, walked and dp-heavy chunks in the order of the 64 counters (3: three waves);
    nothing may carry over from one chunk to the next (the tables, col_dirty, the lists).  The second call takes them in the order of the
    `order` table."""
    k = sc.case(T, W)
    _no_switches(monkeypatch)
    monkeypatch.setenv("CORNETTO_SIFT_BLOCKS", blocks)
    asm = dacc.asm_upload(k.seqs)
    try:
        first, again = _t(dacc.sdust(asm, T, W)), _t(dacc.sdust(asm, T, W))
    finally:
        asm.close()
    assert first == k.exp, (T, W, blocks, _first_diff(first, k.exp))
    assert again == k.exp, (T, W, blocks, "second call", _first_diff(again, k.exp))


def test_product_with_the_smallest_share():
    """the product twin of the test above: set_share(10), the smallest share the library takes (below 10 it answers CORNETTO_E_ARG — asserted
    here), without boost, leaves the kernel a tenth of the chip's wave slots, which take the 2500 chunks of 4.5 Mbases between them.  The kernel
    does not report how many waves ran or how many chunks each took, so this asserts the intervals only: that a wave took several chunks
    follows from the chunk count and the slots a tenth of the device has, it is not measured."""
    import cornetto_amd
    k = sc.twin()
    a = cornetto_amd.Accel(0)
    try:
        with pytest.raises(cornetto_amd.AccelError):
            a.set_share(1)
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


# ---- e. row capacity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name,launches", [("dense", 2), ("56", 1), ("57", 2)])
def test_row_capacity(monkeypatch, name, launches, dev):
    """the first attempt gives a chunk max(16, 1792 / 32) = 56 rows: a chunk with exactly 56 fits (one launch), one with 57 does not (the
    kernel counts on, the host sizes the rows by the fullest chunk and launches again), nothing is truncated.  In the 56-row case the next
    chunk's first interval starts exactly at the chunk's end - W: recorded by both chunks it would be the 57th row.  A fresh handle per
    case: the capacity is raised to what a handle's workspace already holds."""
    import cornetto_amd
    _no_switches(monkeypatch)
    k = sc.cap_dense() if name == "dense" else sc.cap_exact(int(name))
    fullest = max(sc.rows_per_chunk(k).values())
    assert fullest == int(name) if name != "dense" else fullest > sc.CAP_ROWS
    a = cornetto_amd.Accel(0, dev=dev)
    try:
        asm = a.asm_upload(k.seqs)
        try:
            n0 = a.launch_count()
            got = _t(a.sdust(asm, k.T, k.W))
            n = a.launch_count() - n0
        finally:
            asm.close()
    finally:
        a.close()
    assert got == k.exp, (name, _first_diff(got, k.exp))
    assert n == launches, (name, n)
