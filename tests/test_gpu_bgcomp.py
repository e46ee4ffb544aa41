"""GPU: BGZF-compressed depth files inflated on the device in front of the two bedgraph readers (cornetto_bgin_feed_src,
cornetto_bgrun_feed_src; csrc/bgin.hip, bgrun.hip, bgtok.hpp, inflate.hip) and `(no)boringbits` on compressed files.  Everything is parity:
with the plain-text feed of the same text, with numpy for the run reader, with the golden stdout of the unmodified reference.

The shapes are the smallest at which the path can go wrong: block seams inside every kind of token and at every kind of token edge, a
block of one byte, an empty block, a block of 65536 bytes, one block per feed (the carry crosses every seam) and all blocks in one feed, a
carry that is longer than what the next feed brings, runs across block seams and across the tile of the expansion kernel.

On the parent commit the ABI tests fail for want of the two entry points and the CLI tests with "The depth files should have 4 columns"."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgcomp_cases as bz
import bgzf_cases as bc
import cornetto_amd
from cornetto_amd import BG_BLOCK, BGRUN_TILE as T, BedgraphFormatError, Bgzf
from helpers import PANEL, golden, panel_argv
from runs_cases import expand_arrays, fmt, to_runs

pytestmark = pytest.mark.gpu
ALL = 1 << 30   # blocks per feed: all of them in one


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def arrays(acc, res):
    """(names, lengths, [(depth, mq depth) per contig], clamped count) of an ingest's result; the coverage is released"""
    cov, names, ncl = res
    try:
        return names, list(cov.lens), [acc.cov_download(cov, c) for c in range(len(names))], ncl
    finally:
        cov.close()


def same_cov(got, ref):
    assert got[0] == ref[0] and got[1] == ref[1] and got[3] == ref[3], (got[0], got[1], got[3], ref[0], ref[1], ref[3])
    for c, ((d, m), (rd, rm)) in enumerate(zip(got[2], ref[2])):
        assert np.array_equal(d, rd) and np.array_equal(m, rm), (c, np.flatnonzero(d != rd)[:5], np.flatnonzero(m != rm)[:5])


# ---- per base -----------------------------------------------------------------------------------------------------------------------------
def seam_pair():
    """two contigs of 3000 and 2500 positions, values above 65535 among them, and the byte offsets of cov-total at which block seams go:
    inside a contig name, inside each numeric field, between a newline and the next line, exactly at a record's end, a block of one
    byte, an empty block, and behind all of them a block of 65536 bytes"""
    rng = np.random.default_rng(11)
    contigs = [(b"contig_name_%d" % c, [int(v) for v in rng.choice([3, 40, 41, 65535, 65536, 123456], size=n, p=[.3, .3, .3, .04, .03, .03])])
               for c, n in enumerate((3000, 2500))]
    t = bz.per_base(contigs)
    q = bz.per_base([(n, [v // 3 for v in x]) for n, x in contigs])
    lines = t.splitlines(True)
    start = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
    f = lines[200].split(b"\t")
    cuts = [start[100] + 5,                                             # inside a contig name
            start[200] + len(f[0]) + 2,                                 # inside the start field
            start[200] + len(f[0]) + 1 + len(f[1]) + 2,                 # inside the end field
            start[200] + len(f[0]) + len(f[1]) + len(f[2]) + 4,         # inside the depth field
            start[300],                                                 # between a newline and the next line
            start[401] - 1,                                             # exactly at a record's end, in front of its newline
            start[450] + 3, start[450] + 4,                             # a block of one byte
            start[500] + 1, start[500] + 1]                             # an empty block
    cuts = [int(c) for c in cuts]
    cuts.append(cuts[-1] + 65536)                                       # a block of 65536 bytes
    assert len(f[3]) >= 3 and cuts[-1] + 1000 < len(t)
    return t, q, cuts


@pytest.fixture(scope="module")
def seams(acc):
    t, q, cuts = seam_pair()
    sizes = bz.sizes_from_cuts(cuts, len(t))
    assert 1 in sizes and 0 in sizes and 65536 in sizes
    bt = bz.bgzf(t, sizes)
    bq = bz.bgzf(q, bz.seeded_sizes(len(q), 4, 1, 9000))
    assert [m[5] for m in bc.members(bt)][:len(sizes)] == sizes
    ref = arrays(acc, acc.bedgraph_ingest([t], [q]))
    assert ref[1] == [3000, 2500] and ref[3] > 0
    return t, q, bt, bq, ref


@pytest.mark.parametrize("per_feed", [1, ALL, 3])
def test_per_base_seams_in_every_token(acc, seams, per_feed):
    t, q, bt, bq, ref = seams
    same_cov(arrays(acc, acc.bedgraph_ingest_src(Bgzf(bt, per_feed), Bgzf(bq, per_feed))), ref)


@pytest.mark.parametrize("per_feed", [1, ALL])
def test_per_base_one_file_compressed_the_other_plain(acc, seams, per_feed):
    t, q, bt, bq, ref = seams
    pieces = lambda x: [x] if per_feed == ALL else [x[i:i + 9973] for i in range(0, len(x), 9973)]
    same_cov(arrays(acc, acc.bedgraph_ingest_src(Bgzf(bt, per_feed), pieces(q))), ref)
    same_cov(arrays(acc, acc.bedgraph_ingest_src(pieces(t), Bgzf(bq, per_feed))), ref)


def test_per_base_a_file_changes_kind_between_feeds(acc, seams):
    """plain pieces first, then the rest of the file as BGZF blocks: the carry moves to the device with the first compressed source"""
    t, q, bt, bq, ref = seams
    L, C = acc.L, cornetto_amd.C
    cut = t.index(b"\n", 30000) + 8        # inside a record
    rest = bz.bgzf(t[cut:], bz.seeded_sizes(len(t) - cut, 6, 1, 5000))
    blocks, resume, broken = cornetto_amd.bgzf_scan(rest)
    comp, bg = acc._text_from(rest), C.c_void_p()
    acc._chk(L.cornetto_bgin_open(acc.h, C.byref(bg)))
    try:
        head = t[:cut]
        a, b = cornetto_amd.BgSrc(head, len(head), None, None, 0), cornetto_amd.BgSrc(q, len(q), None, None, 0)
        acc._chk(L.cornetto_bgin_feed_src(acc.h, bg, C.byref(a), C.byref(b), 2))
        a = cornetto_amd.BgSrc(None, 0, comp, blocks.ctypes.data, len(blocks))
        acc._chk(L.cornetto_bgin_feed_src(acc.h, bg, C.byref(a), None, 3))
        assert L.cornetto_bgin_done(bg)
        cov, nc, names, ncl = C.c_void_p(), C.c_int32(), C.POINTER(C.c_char_p)(), C.c_int64()
        acc._chk(L.cornetto_bgin_finish(acc.h, bg, C.byref(cov), C.byref(nc), C.byref(names), C.byref(ncl)))
        same_cov(arrays(acc, acc._ingested(cov, nc, names, ncl)), ref)
    finally:
        L.cornetto_bgin_close(acc.h, bg)
        L.cornetto_text_free(acc.h, comp)


@pytest.mark.parametrize("first", ["tot", "mq"])
def test_the_carry_stays_on_the_device_and_is_counted(acc, seams, first):
    """all of one file in three feeds before any of the other: nothing is consumed, cornetto_bgin_pending() is the inflated bytes so far; the
    second feed brings less than the first left behind (the carry is longer than the new bytes)"""
    t, q, bt, bq, ref = seams
    blob, text = (bt, t) if first == "tot" else (bq, q)
    isize = [m[5] for m in bc.members(blob)]
    n = len(isize)
    groups = [n - 2, 1, 1]                  # all but the last block with bytes; that block; the EOF block
    assert sum(isize[:n - 2]) > isize[n - 2] > 0 and isize[n - 1] == 0
    lead, other = Bgzf(blob, groups), Bgzf(bq if first == "tot" else bt, [0, 0, 0])
    pending = []
    got = arrays(acc, acc.bedgraph_ingest_src(lead if first == "tot" else other, other if first == "tot" else lead, pending=pending))
    same_cov(got, ref)
    want = [sum(isize[:n - 2]), len(text), len(text)]
    col = 0 if first == "tot" else 1
    assert [p[col] for p in pending[:3]] == want and [p[1 - col] for p in pending[:3]] == [0, 0, 0], pending[:4]
    assert len(pending) == 4


def test_more_than_a_feed_may_hold_is_refused_before_anything_runs(acc):
    """the limit counts carried plus inflated bytes: 61441 blocks that say 65536 bytes each are more than 0xF0000000"""
    L, C = acc.L, cornetto_amd.C
    one = bz.bgzf(b"c\t0\t1\t5\n", [8])
    blocks, _, _ = cornetto_amd.bgzf_scan(one)
    many = np.repeat(blocks[:1], 61441)
    many["n_dst"] = 65536
    comp, bg = acc._text_from(one), C.c_void_p()
    acc._chk(L.cornetto_bgin_open(acc.h, C.byref(bg)))
    try:
        a = cornetto_amd.BgSrc(None, 0, comp, many.ctypes.data, len(many))
        assert L.cornetto_bgin_feed_src(acc.h, bg, C.byref(a), None, 0) == -3
        many["n_dst"] = 65537
        a = cornetto_amd.BgSrc(None, 0, comp, many.ctypes.data, 1)
        assert L.cornetto_bgin_feed_src(acc.h, bg, C.byref(a), None, 0) == -3        # a block that says more than 65536 bytes
        both = cornetto_amd.BgSrc(b"x", 1, comp, blocks.ctypes.data, 1)
        assert L.cornetto_bgin_feed_src(acc.h, bg, C.byref(both), None, 0) == -3     # plain bytes and blocks in one source
    finally:
        L.cornetto_bgin_close(acc.h, bg)
        L.cornetto_text_free(acc.h, comp)


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------
def runs_pair():
    rng = np.random.default_rng(21)
    def contig(name, n_runs, head):
        recs, p = [], 0
        for ln, v in head + [(int(rng.integers(1, 200)), int(rng.choice([0, 7, 65535, 70000, 31]))) for _ in range(n_runs)]:
            recs.append((name, p, p + ln, v))
            p += ln
        return recs, p
    a, na = contig(b"contig_name_0", 150, [(T - 3, 4), (7, 5), (2 * T + 5, 6)])       # runs that end around and span the tiles of the expansion
    b, nb = contig(b"contig_name_1", 100, [(100, 70000), (T, 3)])
    t = fmt(a + b)
    q = fmt([(b"contig_name_0", p, min(p + 37, na), (p // 37) % 50) for p in range(0, na, 37)] + [(b"contig_name_1", 0, nb, 9)])
    return t, q


@pytest.fixture(scope="module")
def run_files():
    t, q = runs_pair()
    tn, ta, tc = expand_arrays(t)
    qn, qa, qc = expand_arrays(q)
    assert tn == qn and [len(x) for x in ta] == [len(x) for x in qa]
    ref = (tn, [len(x) for x in ta], list(zip(ta, qa)), tc + qc)
    # seams inside names and numbers, between records, a block of one byte and an empty one: sizes of 0 .. 60 bytes cut every record of cov-total
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 61, size=2 * len(t) // 30)]
    sizes = sizes[:next(i for i in range(len(sizes)) if sum(sizes[:i + 1]) >= len(t))]
    assert 0 in sizes and 1 in sizes
    return t, q, bz.bgzf(t, sizes), bz.bgzf(q, bz.seeded_sizes(len(q), 8, 1, 700)), ref


@pytest.mark.parametrize("per_feed", [1, ALL])
@pytest.mark.parametrize("alternate", [True, False])
def test_runs_seams_blocks_and_tiles(acc, run_files, per_feed, alternate):
    t, q, bt, bq, ref = run_files
    same_cov(arrays(acc, acc.bedgraph_runs_ingest_src(Bgzf(bt, per_feed), Bgzf(bq, per_feed), alternate=alternate)), ref)
    if per_feed == 1:
        return
    same_cov(arrays(acc, acc.bedgraph_runs_ingest_src(Bgzf(bt, 7), [q[:1000], q[1000:]], alternate=alternate)), ref)
    same_cov(arrays(acc, acc.bedgraph_runs_ingest_src([t], Bgzf(bq, 5), alternate=alternate)), ref)


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def error_of(fn, *a, **kw):
    with pytest.raises(BedgraphFormatError) as ei:
        fn(*a, **kw)[0].close()
    e = ei.value
    return (e.kind, e.file, e.record, e.a, e.b)


def small_blocks(text, seed):
    return bz.bgzf(text, bz.seeded_sizes(len(text), seed, 1, 40)) if text else bz.bgzf(b"", [])


GOOD = [(b"c1", 0, 40, 5), (b"c1", 40, 90, 7), (b"c2", 0, 3, 70000), (b"c2", 3, 200, 1)]


def swap(i, rec):
    return GOOD[:i] + [rec] + GOOD[i + 1:]


RUN_CHECKS = [        # the cases of tests/test_gpu_runs.py::test_every_check_through_the_abi
    (b"track type=bedGraph\n" + fmt(GOOD), fmt(GOOD), (1, 0, 0, 1, 0)),
    (fmt(GOOD), fmt(GOOD[:2]) + b"c2\t0\t3\t1.5\n", (2, 1, 2, 3, 0)),
    (fmt(GOOD), fmt(GOOD) + b"c3 0", (2, 1, 4, 2, 0)),
    (fmt(GOOD) + b"c3 x 1", fmt(GOOD), (1, 0, 4, 1, 0)),
    (fmt(swap(2, (b"c2", 1, 3, 9))), fmt(GOOD), (6, 0, 2, 1, 0)),
    (fmt(GOOD), fmt(swap(1, (b"c1", 50, 90, 7))), (7, 1, 1, 40, 50)),
    (fmt(swap(1, (b"c1", 30, 90, 7))), fmt(GOOD), (7, 0, 1, 40, 30)),
    (fmt(swap(3, (b"c2", 3, 3, 1))), fmt(GOOD), (8, 0, 3, 3, 3)),
    (fmt(GOOD), fmt(swap(0, (b"c1", 0, 40, -2))), (9, 1, 0, -2, 0)),
    (fmt(GOOD), fmt(GOOD[:2]), (10, 0, 1, 200, 0)),
    (fmt(GOOD[:2]), fmt(GOOD), (10, 0, 1, 0, 200)),
    (fmt(GOOD), fmt(GOOD[:2] + [(b"cX", 0, 200, 1)]), (10, 0, 1, 200, 200)),
    (fmt(GOOD), fmt(swap(1, (b"c1", 40, 91, 7))), (10, 0, 0, 90, 91)),
]


def test_every_check_of_the_run_reader_from_blocks(acc):
    for k, (t, q, want) in enumerate(RUN_CHECKS):
        assert error_of(acc.bedgraph_runs_ingest, [t], [q]) == want, k
        for per_feed in (1, ALL):
            assert error_of(acc.bedgraph_runs_ingest_src, Bgzf(small_blocks(t, k), per_feed), Bgzf(small_blocks(q, 50 + k), per_feed)) == want, (k, per_feed)
    cov, names, ncl = acc.bedgraph_runs_ingest_src(Bgzf(bz.bgzf(b"", [0])), Bgzf(bz.bgzf(b" \n", [1])))
    assert (list(cov.lens), names, ncl) == ([], [], 0)
    cov.close()


def test_every_check_of_the_per_base_reader_from_blocks(acc):
    """the cases of tests/test_gpu_parity.py::test_bedgraph_ingest_errors on a text of 200 records"""
    vals = [(b"ptg000001l", [30 + i % 9 for i in range(120)]), (b"ptg000002l", [12] * 80)]
    tl, ql = bz.per_base(vals).splitlines(True), bz.per_base([(n, [v // 2 for v in x]) for n, x in vals]).splitlines(True)
    cases = [
        ([b"track type=bedGraph\n"] + tl, [b"track type=bedGraph\n"] + ql),
        (tl, ql[:150]),
        (tl, ql[:40] + ql[41:]),
        (tl[:20] + tl[21:], ql[:20] + ql[21:]),
        ([b"ptg000001l\t0\t5\t30\n"], [b"ptg000001l\t0\t5\t30\n"]),
        (tl + [b"ptg000001l\t7\n"], ql + [b"ptg000001l\t7\t8\t1\n"]),
        (tl[:50] + [b"x\t1\t2\tabc\n"], ql[:51]),
        (tl[:51], ql[:50] + [b"ptg000001l\t50\t51\n"]),
    ]
    kinds = set()
    for k, (tt, qq) in enumerate(cases):
        tt, qq = b"".join(tt), b"".join(qq)
        want = error_of(acc.bedgraph_ingest, [tt], [qq])
        kinds.add(want[0])
        for per_feed in (1, ALL):
            assert error_of(acc.bedgraph_ingest_src, Bgzf(small_blocks(tt, k), per_feed), Bgzf(small_blocks(qq, 70 + k), per_feed)) == want, (k, per_feed, want)
    assert kinds == {1, 2, 3, 4, 5}
    # extra cov-mq records are ignored, as ever
    same_cov(arrays(acc, acc.bedgraph_ingest_src(Bgzf(small_blocks(b"".join(tl[:150]), 1), 9), Bgzf(small_blocks(b"".join(ql), 2), 9))),
             arrays(acc, acc.bedgraph_ingest([b"".join(tl[:150])], [b"".join(ql)])))


def damaged_case():
    """a per-base pair (it is a run-length pair too: unit runs) of 900 records, cov-total in blocks of about 400 bytes, block 5 damaged"""
    vals = [(b"ctgA", [20 + i % 13 for i in range(600)]), (b"ctgB", [9] * 300)]
    t, q = bz.per_base(vals), bz.per_base([(n, [v // 2 for v in x]) for n, x in vals])
    blob = bz.bgzf(t, bz.seeded_sizes(len(t), 2, 300, 500))
    assert len(bc.members(blob)) > 9
    return t, q, blob


@pytest.mark.parametrize("per_feed", [1, ALL])
@pytest.mark.parametrize("reader", ["per_base", "runs"])
def test_a_damaged_block_is_reported_with_its_index_and_offset(acc, per_feed, reader):
    t, q, blob = damaged_case()
    ingest = acc.bedgraph_ingest_src if reader == "per_base" else acc.bedgraph_runs_ingest_src
    k = 5
    src = bz.block_offset(blob, k)[1]
    for name, bad in bz.damaged(blob, k):
        assert error_of(ingest, Bgzf(bad, per_feed), [q]) == (BG_BLOCK, 0, k, src, 0), name
        assert error_of(ingest, [t], Bgzf(bad, per_feed)) == (BG_BLOCK, 1, k, src, 0), name      # (the same bytes as the other file: the block is what is reported)
    # the handle is as good as new
    same_cov(arrays(acc, ingest(Bgzf(blob, per_feed), [q])), arrays(acc, acc.bedgraph_ingest([t], [q])))


@pytest.mark.parametrize("per_feed", [1, ALL])
@pytest.mark.parametrize("reader", ["per_base", "runs"])
def test_a_text_error_in_front_of_the_damaged_block_wins_and_one_behind_it_is_never_seen(acc, per_feed, reader):
    t, q, _ = damaged_case()
    ingest, plain = (acc.bedgraph_ingest_src, acc.bedgraph_ingest) if reader == "per_base" else (acc.bedgraph_runs_ingest_src, acc.bedgraph_runs_ingest)
    lines = t.splitlines(True)
    sizes = bz.seeded_sizes(len(t), 2, 300, 500)
    k = 5
    first_of_k, end_of_k = sum(sizes[:k]), sum(sizes[:k + 1])
    # the records that lie wholly in front of block k / wholly behind it
    ends = np.cumsum([len(x) for x in lines])
    in_front = int(np.searchsorted(ends, first_of_k, side="right")) - 2
    behind = int(np.searchsorted(ends, end_of_k, side="right")) + 2
    for at, wins in ((in_front, True), (behind, False)):
        f = lines[at].split(b"\t")
        # end = start: the pair is out of step there (per base: check 3) / a run without positions (check 8).  The line may lose a byte: the
        # records chosen keep a line's distance from block k
        bad_text = b"".join(lines[:at] + [b"\t".join([f[0], f[1], f[1], f[3]])] + lines[at + 1:])
        blob = bz.bgzf(bad_text, sizes)
        want = error_of(plain, [bad_text], [q])
        assert want[0] in (3, 8) and want[2] == at
        assert error_of(ingest, Bgzf(blob, per_feed), [q]) == want              # without damage: the text error, as from the plain file
        for name, bad in bz.damaged(blob, k):
            got = error_of(ingest, Bgzf(bad, per_feed), [q])
            assert got == (want if wins else (BG_BLOCK, 0, k, bz.block_offset(blob, k)[1], 0)), (name, at, got)


# ---- workspaces ---------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_workspaces_held(seams, run_files):
    import selftest_bind as st
    dacc = cornetto_amd.Accel(0, dev=True)
    try:
        t, q, bt, bq, ref = seams
        rt, rq, rbt, rbq, rref = run_files
        same_cov(arrays(dacc, dacc.bedgraph_ingest_src(Bgzf(bt, 3), Bgzf(bq, 3))), ref)
        same_cov(arrays(dacc, dacc.bedgraph_runs_ingest_src(Bgzf(rbt, 50), Bgzf(rbq, 5))), rref)
        for byte in (0xFF, 0xA5):
            filled, skipped, pinned = st.ws_fill(dacc, byte)
            assert {"WS_BG_TEXT_A", "WS_BG_TOK_A", "WS_BZ_BLOCKS", "WS_BZ_STATUS", "WS_BZ_PACK"} <= set(filled), sorted(filled)
            same_cov(arrays(dacc, dacc.bedgraph_ingest_src(Bgzf(bt, 3), Bgzf(bq, 3))), ref)
            st.ws_fill(dacc, byte)
            same_cov(arrays(dacc, dacc.bedgraph_runs_ingest_src(Bgzf(rbt, 50), Bgzf(rbq, 5))), rref)
    finally:
        dacc.close()


# ---- the CLI on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def run(cli, args, env=None):
    e = dict(os.environ)
    for k in ("CORNETTO_ACCEL", "CORNETTO_BGZF", "CORNETTO_BG_PIECE", "CORNETTO_DEVICES"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgcomp_gpu")
    texts = {fn: bz.golden_text(golden_dir, fn) for fn in bz.DEPTH_FILES}
    return bz.write_variants(d, texts, seed=3), bz.write_variants(d, {fn: to_runs(x, "max") for fn, x in texts.items()}, seed=5, lo=1, hi=900, tag="runs.")


MODES = {
    "bgzf_dozens_of_rounds": ("bgzf", {"CORNETTO_BG_PIECE": "32768"}),
    "bgzf_default_piece": ("bgzf", {}),
    "bgzf_through_zlib": ("bgzf", {"CORNETTO_BGZF": "0"}),
    "gzip": ("gzip", {}),
    "gzip_small_piece": ("gzip", {"CORNETTO_BG_PIECE": "50000"}),
}
GOLDEN = [PANEL[4], PANEL[5], PANEL[14]]          # noboringbits and boringbits on cov-*, boringbits on sparse-*


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_goldens_from_compressed_files(cli, golden_dir, files, mode):
    per_base, runs = files
    kind, env = MODES[mode]
    for args, exp in GOLDEN:
        rc, out, err = run(cli, panel_argv(per_base[kind], args), env)
        assert rc == 0, err.decode()
        assert out == golden(golden_dir, exp), (mode, exp)
    a = panel_argv(runs[kind], GOLDEN[0][0])
    rc, out, err = run(cli, a[:1] + ["--runs"] + a[1:], env)
    assert rc == 0, err.decode()
    assert out == golden(golden_dir, GOLDEN[0][1])


@pytest.mark.parametrize("which", ["t", "q"])
def test_cli_one_file_compressed_the_other_plain(cli, golden_dir, files, which):
    per_base, runs = files
    pick = lambda v: {fn: (v["bgzf"][fn] if ("total" in fn) == (which == "t") else v["plain"][fn]) for fn in v["plain"]}
    args, exp = GOLDEN[0]
    for env in ({"CORNETTO_BG_PIECE": "100000"}, {}):
        rc, out, err = run(cli, panel_argv(pick(per_base), args), env)
        assert rc == 0 and out == golden(golden_dir, exp), err.decode()
        a = panel_argv(pick(runs), args)
        rc, out, err = run(cli, a[:1] + ["--runs"] + a[1:], env)
        assert rc == 0 and out == golden(golden_dir, exp), err.decode()


def test_cli_panel_from_compressed_files(cli, files, tmp_path):
    per_base, _ = files
    lens = {}
    for ln in open(per_base["plain"]["cov-total.bg"], "rb"):
        f = ln.split()
        lens[f[0]] = int(f[2])
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, ln) for n, ln in lens.items()))
    opts = ["-w", "1000", "-i", "100", "-e", "2000", "-m", "10000", "--panel", str(tmp_path / "asm.bed"), "--panel-params", "300,2000,500,700,3000,2500,4000"]
    want = run(cli, ["noboringbits", per_base["plain"]["cov-total.bg"], "-q", per_base["plain"]["cov-mq20.bg"]] + opts)
    assert want[0] == 0 and want[1]
    for kind in ("bgzf", "gzip"):
        got = run(cli, ["noboringbits", per_base[kind]["cov-total.bg"], "-q", per_base[kind]["cov-mq20.bg"]] + opts, {"CORNETTO_BG_PIECE": "200000"})
        assert got[:2] == want[:2], got[2].decode()


SMALL_ARGS = ["-w", "100", "-i", "10", "-m", "500", "-e", "100"]


def small_pair():
    vals = [(b"ctgA", [30 + (i * 7) % 11 for i in range(3000)]), (b"ctgB", [70000 if i == 5 else 12 for i in range(1500)])]
    return bz.per_base(vals), bz.per_base([(n, [v // 2 for v in x]) for n, x in vals])


def test_cli_damaged_truncated_and_mixed_chains(cli, tmp_path):
    t, q = small_pair()
    (tmp_path / "q.bg").write_bytes(q)
    blob = bz.bgzf(t, bz.seeded_sizes(len(t), 1, 500, 3000), eof=False)
    k = 3
    off, _ = bz.block_offset(blob, k)
    bad = dict(bz.damaged(blob, k)[::3])                                  # the footer's CRC, a payload byte
    bad["cut"] = blob[:off + 40]
    bad["gzip_behind"] = blob + gzip.compress(b"ctgB\t1500\t1501\t3\n")
    for name, data in bad.items():
        p = tmp_path / ("bad_%s.bg.gz" % name)
        p.write_bytes(data)
        for extra in ([], ["--runs"])[:2 if name == "crc" else 1]:
            rc, out, err = run(cli, ["noboringbits", str(p), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS + extra, {"CORNETTO_BG_PIECE": "20000"})
            lines = [ln for ln in bz.stderr_lines(err) if "ERROR" in ln]
            assert rc == 1 and out == b"" and len(lines) == 1 and os.path.basename(str(p)) in lines[0], (name, extra, rc, lines)
            if name != "gzip_behind":
                assert "block %d at offset %d" % (k, off) in lines[0], (name, lines)
    # a file without the EOF block is accepted
    (tmp_path / "t.bg").write_bytes(t)
    (tmp_path / "noeof.bg.gz").write_bytes(blob)
    want = run(cli, ["noboringbits", str(tmp_path / "t.bg"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS)
    got = run(cli, ["noboringbits", str(tmp_path / "noeof.bg.gz"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS)
    assert want[0] == 0 and want[1] and got[:2] == want[:2] and bz.stderr_lines(got[2]) == bz.stderr_lines(want[2])


def test_cli_text_errors_read_as_for_the_plain_file(cli, tmp_path):
    t, q = small_pair()
    tl, ql = t.splitlines(True), q.splitlines(True)
    cases = {
        "columns": (b"".join(tl[:700] + [b"ctgA\t700\t701\n"] + tl[701:]), q),
        "order": (t, b"".join(ql[:900] + ql[901:])),
        "increment": (b"".join(tl[:1200] + tl[1201:]), b"".join(ql[:1200] + ql[1201:])),
        "end": (b"".join(tl[:40] + [b"ctgA\t40\t45\t3\n"] + tl[41:]), b"".join(ql[:40] + [b"ctgA\t40\t45\t3\n"] + ql[41:])),
    }
    for name, (tt, qq) in cases.items():
        v = bz.write_variants(tmp_path, {"total.bg": tt, "mq20.bg": qq}, seed=9, lo=1, hi=700, tag=name + ".")
        want = run(cli, ["noboringbits", v["plain"]["total.bg"], "-q", v["plain"]["mq20.bg"]] + SMALL_ARGS)
        assert want[0] == 1 and want[1] == b"" and any("ERROR" in ln for ln in bz.stderr_lines(want[2])), name
        for kind in ("bgzf", "gzip")[:2 if name == "order" else 1]:
            got = run(cli, ["noboringbits", v[kind]["total.bg"], "-q", v[kind]["mq20.bg"]] + SMALL_ARGS, {"CORNETTO_BG_PIECE": "9000"})
            # (the name in front of ::ERROR is the function that printed the line: the same message, the same numbers)
            msg = lambda e: [ln.split("ERROR]", 1)[1] for ln in bz.stderr_lines(e) if "ERROR]" in ln]
            assert got[:2] == want[:2] and msg(got[2]) == msg(want[2]) and len(msg(got[2])) == 1, (name, kind, got[2].decode())


def test_cli_compressed_files_on_two_devices(cli, golden_dir, files):
    if cornetto_amd.lib().cornetto_accel_device_count() < 2:
        pytest.skip("needs two visible GPUs")
    per_base, runs = files
    args, exp = GOLDEN[0]
    rc, out, err = run(cli, panel_argv(per_base["bgzf"], args), {"CORNETTO_DEVICES": "0,1"})
    assert rc == 0 and out == golden(golden_dir, exp), err.decode()
