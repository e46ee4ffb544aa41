"""GPU: the add-scans of the library (csrc/wave.hpp, scan.hpp, the 64-bit scan of bgrun.hip, the look-backs of ivlmerge.hpp's fused merge)
on their own, through the cn_selftest_* entry points of the development build (selftest_bind.py), against numpy: cumsum in uint64,
reduced mod 2^32 for the 32-bit scans.  What the product entry points cannot reach: the walk of the look-back over PREPARED tile states
(on real inputs, which path it takes is decided by timing), strided and multi-counter scans at more than one tile, the host's bookkeeping
(epochs instead of clearing, the reset when the work space grows or the epoch wraps), full-range values."""
import numpy as np
import pytest

import cornetto_amd
import oracle_bind as ob
import selftest_bind as sb

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1
EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)       # the row (16 lanes) and bank (32) edges of the DPP steps
TILE = 4096                                        # cnscan::SC_TILE


def excl_cumsum(x):
    """(exclusive prefixes, total) in uint64 (wraps mod 2^64, as the 64-bit scan does)"""
    x = x.astype(np.uint64)
    inc = np.cumsum(x, dtype=np.uint64)
    return inc - x, int(inc[-1]) if len(x) else 0


def value_sets_u32(rng, n, group):
    """the value sets of the primitives: n values, scanned in groups of `group`"""
    sets = {"zeros": np.zeros(n, np.uint32), "ones": np.ones(n, np.uint32),
            "below_2_16": rng.integers(0, 1 << 16, n, dtype=np.uint32),
            "full_range": rng.integers(0, 1 << 32, n, dtype=np.uint32)}         # sums wrap mod 2^32 (wave_incl_dpp adds as int)
    for lane in EDGE_LANES:                            # one non-zero per group, in wave `g mod (group / 64)` of group g
        v = np.zeros(n, np.uint32)
        for g in range(n // group):
            v[g * group + (g % (group // 64)) * 64 + lane] = rng.integers(1, 1 << 32)
        sets["single_lane_%d" % lane] = v
    return sets


def value_sets_u64(rng, n, group):
    sets = {"zeros": np.zeros(n, np.uint64), "ones": np.ones(n, np.uint64),
            "above_2_32": rng.integers(1 << 32, 1 << 44, n, dtype=np.uint64),
            "full_range": rng.integers(0, 1 << 64, n, dtype=np.uint64)}         # sums wrap mod 2^64
    for lane in EDGE_LANES:
        v = np.zeros(n, np.uint64)
        for g in range(n // group):
            v[g * group + (g % (group // 64)) * 64 + lane] = rng.integers(1 << 32, 1 << 63)
        sets["single_lane_%d" % lane] = v
    return sets


# ---- 1. wave and block primitives -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [sb.WAVE_INCL_U32, sb.WAVE_INCL_U64, sb.WAVE_INCL_DPP, sb.WAVE_SUM], ids=["wave_incl_u32", "wave_incl_u64", "wave_incl_dpp", "wave_sum"])
def test_wave_primitives_against_cumsum(dacc, which):
    rng = np.random.default_rng(100 + which)
    n = 64 * 13                                        # 13 waves: workgroups of 4 waves and a last one of 1
    sets = value_sets_u64(rng, n, 64) if which == sb.WAVE_INCL_U64 else value_sets_u32(rng, n, 64)
    for name, v in sets.items():
        got = sb.wave(dacc, which, v)
        w = v.reshape(-1, 64).astype(np.uint64)
        inc = np.cumsum(w, axis=1, dtype=np.uint64)
        if which == sb.WAVE_SUM:
            exp = np.repeat(inc[:, 63:], 64, axis=1)
        else:
            exp = inc
        if which != sb.WAVE_INCL_U64:
            exp = exp & np.uint64(M32)
        assert np.array_equal(got.astype(np.uint64), exp.reshape(-1)), name


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("is64", [False, True], ids=["u32", "u64"])
def test_block_excl_against_cumsum(dacc, threads, is64):
    rng = np.random.default_rng(200 + threads + is64)
    n = threads * 5
    sets = value_sets_u64(rng, n, threads) if is64 else value_sets_u32(rng, n, threads)
    for name, v in sets.items():
        pre, tot = sb.block_excl(dacc, threads, v)
        b = v.reshape(-1, threads).astype(np.uint64)
        inc = np.cumsum(b, axis=1, dtype=np.uint64)
        exp_pre, exp_tot = inc - b, inc[:, -1]
        if not is64:
            exp_pre, exp_tot = exp_pre & np.uint64(M32), exp_tot & np.uint64(M32)
        assert np.array_equal(pre.astype(np.uint64), exp_pre.reshape(-1)), name
        assert np.array_equal(tot.astype(np.uint64), exp_tot), name


# ---- 2. the walk of the look-back over prepared states --------------------------------------------------------------------------------

def word(kind, epoch, value):
    return (int(kind) << 62) | (int(epoch) << 32) | int(value)


def prepared_states(rng, tile, K, epoch, far_stale, n_tiles):
    """(kind, epoch, value) of n_tiles tiles as the walk of `tile` finds them: the K nearest predecessors have published their own total
    (kind 1), the one in front of them its inclusive prefix (kind 2; none when K == tile).  Everything further away that the SAME round
    of 64 polls is ready too, with values that must not be counted; what no round reaches is zero, or a word of the epoch before."""
    kind = np.zeros(n_tiles, np.int64)
    ep = np.zeros(n_tiles, np.int64)
    val = rng.integers(0, 1 << 32, n_tiles, dtype=np.uint64).astype(np.int64)
    if far_stale:
        kind[:] = rng.integers(1, 3, n_tiles)
        ep[:] = epoch - 1
    else:
        val[:] = 0
    stop = tile - 1 - K                                # -1: none
    lo_round = max(0, tile - 64 * (K // 64 + 1))       # the lowest tile that the round which meets `stop` polls
    if stop >= 0:
        kind[lo_round:stop] = rng.integers(1, 3, stop - lo_round)
        ep[lo_round:stop] = epoch
        val[lo_round:stop] = rng.integers(1 << 31, 1 << 32, stop - lo_round)
        kind[stop], ep[stop] = 2, epoch
        val[stop] = rng.integers(1 << 31, 1 << 32)
    kind[stop + 1:tile], ep[stop + 1:tile] = 1, epoch
    val[stop + 1:tile] = rng.integers(1 << 31, 1 << 32, tile - stop - 1)
    # the tile itself: whatever an earlier call left; the tiles behind it: not the walk's business
    kind[tile:], ep[tile:] = rng.integers(0, 3, n_tiles - tile), max(epoch - 1, 0)
    val[tile:] = rng.integers(0, 1 << 32, n_tiles - tile)
    return kind, ep, val


def protocol_excl(kind, ep, val, tile, epoch):
    """the documented protocol, not the loop: the sum in front of `tile` is the inclusive prefix of the NEAREST predecessor that has one
    (this epoch), plus the own totals of the tiles between it and `tile`; with no such predecessor, the totals of all tiles in front"""
    known = [t for t in range(tile) if kind[t] == 2 and ep[t] == epoch]
    first = known[-1] if known else 0
    assert all(ep[t] == epoch and (kind[t] == 1 or t == first and known) for t in range(first, tile))
    return int(sum(int(val[t]) for t in range(first, tile))) & M32


WALK_CASES = [(0, 0), (1, 0), (1, 1), (5, 5), (63, 63), (64, 63), (64, 64), (65, 0), (65, 63), (65, 64), (65, 65), (130, 0), (130, 64),
              (130, 127), (130, 128), (130, 129), (130, 130), (200, 70)]


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("tile,K", WALK_CASES)
def test_lookback_walk_over_prepared_states(dacc, tile, K, stride):
    """(tile, K): the K nearest predecessors hold their own totals, tile - 1 - K holds its inclusive prefix (K == tile: nobody does, the
    walk runs into the sentinel lanes).  K >= 64 takes a second, K >= 128 a third round of 64; K % 64 is the lane of the stop.
    A walk that counted `lane < first` instead of `lane <= first` loses the inclusive prefix (>= 2^31 here) in every case with K < tile;
    one that dropped a round, or counted lanes beyond the stop, misses or adds values >= 2^31."""
    rng = np.random.default_rng(1000 * tile + 10 * K + stride)
    n_tiles = tile + 3
    for epoch in (1, 0x2AAAAAAA, 0x3FFFFFFF):
        for far_stale in (False, True):
            kind, ep, val = prepared_states(rng, tile, K, epoch, far_stale, n_tiles)
            own = int(rng.integers(0, 1 << 32))
            words = rng.integers(1, 1 << 64, n_tiles * stride, dtype=np.uint64)       # the neighbours of a state in its record: poison
            for t in range(n_tiles):
                words[t * stride + stride - 1] = word(kind[t], ep[t], val[t])
            exp_excl = protocol_excl(kind, ep, val, tile, epoch)
            exp_words = words.copy()
            exp_words[tile * stride + stride - 1] = word(2, epoch, (exp_excl + own) & M32)
            rc, excl = sb.walk_rc(dacc, words, stride, tile, epoch, own)
            assert rc == 0, (epoch, far_stale)
            assert excl == exp_excl, (epoch, far_stale, hex(excl), hex(exp_excl))
            assert np.array_equal(words, exp_words), (epoch, far_stale, np.flatnonzero(words != exp_words))


@pytest.mark.parametrize("bad", ["kind_0", "other_epoch", "second_round"])
def test_the_walk_guard_refuses_a_state_that_is_not_ready(dacc, bad):
    """a word that is not ready would make the wave wait for a writer that does not exist: the entry point checks on the host and launches
    nothing (the words come back untouched, the state of the tile included)"""
    epoch, tile = 7, 70
    words = np.array([word(1, epoch, t + 1) for t in range(tile + 1)], dtype=np.uint64)
    if bad == "kind_0":
        words[tile - 3] = word(0, epoch, 5)
    elif bad == "other_epoch":
        words[tile - 1] = word(2, epoch - 1, 5)
    else:
        words[2] = 0                                   # polled by the second round only
    before = words.copy()
    rc, _ = sb.walk_rc(dacc, words, 1, tile, epoch, 9)
    assert rc == sb.E_ARG
    assert np.array_equal(words, before)


# ---- 3. the whole scan ----------------------------------------------------------------------------------------------------------------

SCAN_N = [1, 4095, 4096, 4097, 8192, 64 * TILE, 64 * TILE + 1, 65 * TILE + 1, 130 * TILE + 5]
SCAN_LAYOUTS = [(1, 1, 0), (1, 2, 1), (2, 2, 0), (4, 4, 0), (3, 4, 0)]           # (m, stride, first): cov_order scans stride 2 from in + 1


def scan_value_sets(rng, n, stride):
    """records of `stride` counters whose per-counter sums stay below 2^32, and one set whose sums do not"""
    small = max(1, min(1 << 16, M32 // n))
    sets = {"zeros": np.zeros(n * stride, np.uint32), "ones": np.ones(n * stride, np.uint32),
            "random": rng.integers(0, small, n * stride, dtype=np.uint32)}
    v = np.zeros((n, stride), np.uint32)               # one non-zero per counter, at the seams of the tiles and of the look-back rounds
    for q, i in enumerate([TILE - 1, 0, TILE, 64 * TILE][:stride]):
        v[min(i, n - 1), q] = M32
    sets["single"] = v.reshape(-1)
    sets["wrapping"] = rng.integers(0, 1 << 32, n * stride, dtype=np.uint32)
    return sets


def check_scan(acc, rec, n, m, stride, first, exact, tag):
    outs, tot = sb.scan_u32(acc, rec, n, stride, first, m)
    r = rec.reshape(n, stride)
    for q in range(m):
        pre, total = excl_cumsum(r[:, first + q])
        assert np.array_equal(outs[q].astype(np.uint64), pre & np.uint64(M32)), (tag, q)
        if exact:                                      # (with a sum of 2^32 or more the total is not exact: scan.hpp, exclusive_u32_multi)
            assert total <= M32 and int(tot[q]) == total, (tag, q)


@pytest.mark.parametrize("m,stride,first", SCAN_LAYOUTS)
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_lookback_against_cumsum(dacc, n, m, stride, first):
    rng = np.random.default_rng(n * 31 + m * 7 + stride)
    for name, rec in scan_value_sets(rng, n, stride).items():
        check_scan(dacc, rec, n, m, stride, first, name != "wrapping", name)


@pytest.mark.parametrize("m,stride", [(1, 1), (4, 4)])
def test_scan_states_of_earlier_epochs_in_higher_tiles(m, stride):
    """one handle: large, small, large, small + 1, twice with other values — the small calls leave the states of the large one in the
    tiles they do not reach, the next large call finds them there with an older epoch"""
    acc = cornetto_amd.Accel(0, dev=True)
    try:
        rng = np.random.default_rng(77 + m)
        for rnd in range(2):
            for n in (130 * TILE + 5, 4097, 130 * TILE + 5, 4098):
                rec = rng.integers(0, M32 // n, n * stride, dtype=np.uint32)
                check_scan(acc, rec, n, m, stride, 0, True, (rnd, n))
    finally:
        acc.close()


def test_scan_work_space_grows_with_tickets_drawn():
    """a fresh handle: the work space of the first call (one tile: 72 bytes and 1/8 head room) holds the two tiles of the second, not the
    three of the third — new, cleared memory and a ticket counter that starts again while the host has handed out 3 tickets; and so on"""
    acc = cornetto_amd.Accel(0, dev=True)
    try:
        rng = np.random.default_rng(78)
        for n in (1, 4097, 2 * TILE + 1, 2 * TILE + 1, 5 * TILE, 12 * TILE + 1, 4097, 66 * TILE, 3):
            for m, stride in ((1, 1), (2, 2)):
                rec = rng.integers(0, M32 // n, n * stride, dtype=np.uint32)
                check_scan(acc, rec, n, m, stride, 0, True, (n, m))
    finally:
        acc.close()


# ---- 4. the epoch wrap ----------------------------------------------------------------------------------------------------------------

def test_scan_epoch_wrap_meets_no_stale_state():
    """64 tiles of A at epoch 1, the epoch set to the last but one, one tile at the last epoch (0x3FFFFFFF), then 64 tiles of B: the states
    A left in tiles 1 .. 63 must not count.  When the epoch simply went round to 1 (before the work space was cleared at the wrap), every
    one of them read "inclusive prefix known, epoch 1", and a tile of B that polled before its predecessor had published again added a
    prefix of A: that failed with high probability, not every time — it depends on who polls when.  With the clearing it cannot fail."""
    acc = cornetto_amd.Accel(0, dev=True)
    try:
        rng = np.random.default_rng(4)
        n = 64 * TILE
        a = rng.integers(1 << 12, 1 << 13, n, dtype=np.uint32)
        b = rng.integers(0, 1 << 12, n, dtype=np.uint32)
        check_scan(acc, a, n, 1, 1, 0, True, "A")
        sb.scan_set_epoch(acc, 0x3FFFFFFE)
        check_scan(acc, np.arange(100, dtype=np.uint32), 100, 1, 1, 0, True, "last epoch")
        check_scan(acc, b, n, 1, 1, 0, True, "B after the wrap")
        check_scan(acc, a, n, 1, 1, 0, True, "A after the wrap")
    finally:
        acc.close()


def _ivls(rng, n, n_ctg, max_len, long_one):
    ctg = np.sort(rng.integers(0, n_ctg, size=n)).astype(np.int32)
    start = rng.integers(0, 5_000_000, size=n).astype(np.int32)
    order = np.lexsort((start, ctg))
    iv = np.zeros(n, cornetto_amd.IVL_DT)
    iv["ctg"], iv["start"] = ctg[order], start[order]
    iv["finish"] = iv["start"] + rng.integers(0, max_len, size=n).astype(np.int32)
    if long_one:
        iv["finish"][n // 3] = iv["start"][n // 3] + 4_000_000
    return iv


def _merge_ref(iv, dist):
    s = np.zeros(len(iv), ob.SPAN_DT)
    s["ctg"], s["start"], s["end"] = iv["ctg"], iv["start"], iv["finish"]
    r = ob.ivl_merge(s, dist)
    out = np.zeros(len(r), cornetto_amd.IVL_DT)
    out["ctg"], out["start"], out["finish"] = r["ctg"], r["start"], r["end"]
    return out


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 65 * 1024 + 1, 130 * 1024 + 5])
def test_fused_merge_against_the_oracle(dacc, n):
    """the one-launch merge (the max walk and the head count's look-back of st_fused) on its own: the public interval merge takes the
    five-launch path, only sdust reaches this one"""
    rng = np.random.default_rng(n)
    for dist, long_one in ((0, False), (50, True)):
        iv = _ivls(rng, n, n // 1000 + 3, 3000, long_one)
        assert np.array_equal(sb.merge_fused(dacc, iv, dist), _merge_ref(iv, dist)), (dist, long_one)
    iv = _ivls(rng, n, 3, 3000, False)
    assert np.array_equal(sb.merge_fused(dacc, iv, 0, n_cap=n + n // 8 + 4096), _merge_ref(iv, 0))      # a grid with tiles beyond the rows


def test_fused_merge_epoch_wrap_meets_no_stale_state():
    """as test_scan_epoch_wrap_meets_no_stale_state for the epoch of the fused merge (both of its look-backs keep epoch-tagged states):
    A has high contig numbers and one interval that swallows many, so its maxima outrank and its head counts differ from B's.  Before
    the work space was cleared at the wrap this failed with high probability, not every time."""
    acc = cornetto_amd.Accel(0, dev=True)
    try:
        rng = np.random.default_rng(5)
        n = 64 * 1024
        a = _ivls(rng, n, 40, 3000, True)
        a["ctg"] += 1000
        b = _ivls(rng, n, 7, 300, False)
        ref_a, ref_b = _merge_ref(a, 0), _merge_ref(b, 0)
        assert np.array_equal(sb.merge_fused(acc, a), ref_a)
        sb.st_set_epoch(acc, 0x3FFFFFFE)
        assert np.array_equal(sb.merge_fused(acc, b[:1000]), _merge_ref(b[:1000], 0))
        assert np.array_equal(sb.merge_fused(acc, b), ref_b)
        assert np.array_equal(sb.merge_fused(acc, a), ref_a)
    finally:
        acc.close()


# ---- 5. the 64-bit scan ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1, 1025 * 2048 + 3])
def test_scan_u64_against_cumsum(dacc, n):
    """tiles of 2048 run lengths; above 1024 tiles every thread of rl_scan_totals takes two tile totals, and the threads behind the last
    pair none"""
    rng = np.random.default_rng(n)
    for name, v in (("above_2_32", rng.integers(1 << 32, 1 << 40, n, dtype=np.uint64)), ("ones", np.ones(n, np.uint64))):
        pre, total = excl_cumsum(v)
        got, got_total = sb.scan_u64(dacc, v)
        assert np.array_equal(got, pre), name
        assert got_total == total, name
