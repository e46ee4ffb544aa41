"""cov_blocks_scan (csrc/cov.hip): the block prefixes of `-i 50` with a window size that is a multiple of it come from wave scans over
the 16-byte vectors in load order, not from the staging kernel's transpose through LDS.  Both kernels must leave the same bytes, so
every case runs on the product build, on the development build, and on the development build with CORNETTO_COV_BLOCKS_STAGE=1 (the
staging kernel forced), and all three must equal the oracle's get_regs() and the exact totals.

All contigs are uploaded as ONE coverage, the odd lengths first: the later contigs then start at element offsets of every residue,
their base addresses 2 mod 4 and 2 mod 16, and each contig's last vector is followed by the next contig's values, not by zeros."""
import numpy as np
import pytest

import cornetto_amd
import oracle_bind as ob

pytestmark = pytest.mark.gpu

TILE = 12_800                       # positions of a block tile at -i 50 (256 blocks); a wave owns 3200 of them, in 7 rounds of 64 vectors
LENS = ([1, 7, 9, 49, 51, 199, 201, 3199, 3201, 6399, 6401, 12_799, 12_801, 25_607, 77_777]           # odd ones first
        + [8, 50, 200, 3200, 12_800]
        + [9600 + 512 * k + 3 for k in range(7)]                 # the contig ends in each of the seven rounds of a tile's last wave
        + [3 * TILE])                                            # no partial tile
WRAP_LEN = 131_072                  # depth = mq = 65535 throughout: the running prefix passes 2^32 near position 65 540, inside a tile

SCAN_PATH = [(2500, 50), (50, 50), (100, 50)]
STAGE_PATH = [(2549, 50), (7, 50)]                               # r = w % inc != 0: heads, the staging kernel


@pytest.fixture(scope="module")
def contigs():
    rng = np.random.default_rng(50)
    depths = [rng.integers(1, 65_536, size=n).astype(np.uint16) for n in LENS]
    mqs = [rng.integers(0, 65_536, size=n).astype(np.uint16) for n in LENS]
    depths.append(np.full(WRAP_LEN, 65_535, np.uint16))
    mqs.append(np.full(WRAP_LEN, 65_535, np.uint16))
    return depths, mqs


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


@pytest.fixture(params=["product", "dev", "dev-stage"])
def build(request, acc, dacc, monkeypatch):
    """the handle of the build under test, the staging kernel forced or not"""
    if request.param == "dev-stage":
        monkeypatch.setenv("CORNETTO_COV_BLOCKS_STAGE", "1")
    else:
        monkeypatch.delenv("CORNETTO_COV_BLOCKS_STAGE", raising=False)
    return acc if request.param == "product" else dacc


_EXPECTED = {}


def expected(contigs, w, inc):
    """the contigs the reference accepts with (w, inc), and the oracle's windows of each: made once per pair"""
    if (w, inc) not in _EXPECTED:
        keep = [i for i, d in enumerate(contigs[0]) if ob.regs_assert(d.size, w, inc) == 0]
        _EXPECTED[(w, inc)] = keep, [ob.get_regs(contigs[0][i], contigs[1][i], w, inc) for i in keep]
    return _EXPECTED[(w, inc)]


@pytest.mark.parametrize("w,inc", SCAN_PATH + STAGE_PATH)
def test_windows_and_totals_vs_oracle(build, contigs, w, inc):
    keep, exp = expected(contigs, w, inc)
    assert keep and (len(keep) == len(contigs[0]) or (w, inc) == (7, 50))          # (w < inc: the reference's asserts end it for most lengths)
    depths, mqs = [contigs[0][i] for i in keep], [contigs[1][i] for i in keep]
    cov = build.cov_upload(depths, mqs)
    try:
        sd, sq, n = build.cov_prepare(cov, w, inc)
        assert sd == sum(int(d.astype(np.int64).sum()) for d in depths)    # exact, beyond 2^32: 131 072 x 65 535 alone is 2^33
        assert sq == sum(int(q.astype(np.int64).sum()) for q in mqs)
        assert n == sum(d.size for d in depths)
        for ci, e in enumerate(exp):
            got = build.cov_regs(cov, ci)
            assert got.size == e.size and np.array_equal(got, e.astype(got.dtype)), (
                "contig %d of %d positions: first difference at window %d" % (ci, depths[ci].size, int(np.flatnonzero(got != e.astype(got.dtype))[0])))
    finally:
        cov.close()


def test_selection_with_windows_whose_int_sums_wrap(build, contigs):
    """-w 70000 -i 50: a window is 1400 blocks, more than five tiles, and its `int` sums wrap as the reference's do — through cov_select, as
    test_cov_select_windows_whose_int_sums_wrap (test_gpu_parity.py) takes it"""
    w, inc = 70_000, 50
    keep, regs = expected(contigs, w, inc)
    assert len(keep) == len(contigs[0])
    depths, mqs = contigs
    cov = build.cov_upload(depths, mqs)
    try:
        build.cov_prepare(cov, w, inc)
        lo, hi, Q, edge, min_len = 100, 64_000, 0.6, 10, 1000
        for boring in (False, True):
            exp = []
            for ci, d in enumerate(depths):
                n = d.size
                if (n > min_len) if boring else (n >= min_len):
                    for r in regs[ci]:
                        st, end, dep, mq = int(r["st"]), int(r["end"]), int(r["depth"]), int(r["mq_depth"])
                        fun = bool(ob.is_fun(dep, mq, lo, hi, Q))
                        if (st > edge and end < n - edge and not fun) if boring else fun:
                            exp.append((ci, st, end, dep, mq))
            recs = build.cov_select(cov, lo, hi, Q, edge, min_len, boring)
            assert [tuple(int(x) for x in r) for r in recs] == exp, boring
    finally:
        cov.close()
