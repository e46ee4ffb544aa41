"""GPU: run-length bedgraphs expanded on the device (csrc/bgrun.hip, cornetto_bgrun_*) and `(no)boringbits --runs`.  The run reader is defined by
expansion, so everything here is parity: with the per-base reader (cornetto_bgin_*) on the expanded text, with the expansion done in numpy,
position by position, and with the golden stdout of the unmodified reference on the per-base fixtures.

The shapes are the smallest at which each part of the expansion kernel can go wrong (T = BGRUN_TILE, the positions one workgroup owns): runs that
end at and around a tile edge, a run over several tiles, a tile full of one-position runs, contig seams inside a tile and on its edge, spans
that start off a 16-byte boundary.  The scan of the run lengths is 64-bit and a feed is one span, so there is no span cutting to force."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import cornetto_amd
from cornetto_amd import BGRUN_TILE as T, BedgraphFormatError
from helpers import PANEL, PANEL_ABORT, golden, panel_argv, token_at
from runs_cases import expand, expand_arrays, fmt, parse, to_runs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    for ref, _, _ in _PER_BASE.values():
        ref.close()
    _PER_BASE.clear()
    a.close()


_PER_BASE = {}   # the per-base reader's coverage of the pair of texts checked last (the tests that feed one pair in many ways share it)


def text_of(contigs, prefix=b"c"):
    """[[(run length, value), ...] per contig] -> run-length bedgraph text"""
    recs = []
    for ci, runs in enumerate(contigs):
        p = 0
        for ln, v in runs:
            recs.append((prefix + b"%d" % ci, p, p + ln, v))
            p += ln
    return fmt(recs)


def recut(contigs, step):
    """the same contig lengths with other run boundaries (every `step` positions) and other values"""
    out = []
    for ci, runs in enumerate(contigs):
        n = sum(ln for ln, _ in runs)
        out.append([(min(step, n - p), (3 * ci + p // step) % 50) for p in range(0, n, step)])
    return out


SHAPES = {
    "one_position": [[(1, 9)]],
    "end_T-1": [[(T - 1, 4), (5, 6)]],
    "end_T": [[(T, 4), (5, 6)]],
    "end_T+1": [[(T + 1, 4), (5, 6)]],
    "one_run_3T+1": [[(3 * T + 1, 33)]],
    "T_unit_runs_then_long": [[(1, i % 7) for i in range(T)] + [(2 * T + 3, 8)]],
    "seam_inside_tile": [[(100, 1), (900, 2)], [(T, 3), (17, 4)]],
    "seam_on_tile_edge": [[(T - 5, 1), (5, 2)], [(T, 3)], [(1, 4)]],
    "contigs_of_one_position": [[(1, i)] for i in range(1, 70)] + [[(T + 1, 5)]] + [[(1, 6)], [(1, 7)]],
    "clamped_values": [[(3, 65535), (T, 65536), (2, 70000), (40, 65534)]],
}


def check_parity(acc, t, q, pieces=None, alternate=True):
    """run ingest of (t, q) against the per-base ingest of their expansion (made once per pair of texts) and against numpy: names, lengths,
    clamp count, the three sums, every position of both arrays"""
    tp, qp = pieces if pieces else ([t], [q])
    cov, names, ncl = acc.bedgraph_runs_ingest(tp, qp, alternate=alternate)
    if (t, q) not in _PER_BASE:
        _PER_BASE.clear()
        _PER_BASE[(t, q)] = acc.bedgraph_ingest([expand(t)], [expand(q)])
    ref, rnames, rncl = _PER_BASE[(t, q)]
    en, ed, ecl_t = expand_arrays(t)
    qn, eq, ecl_q = expand_arrays(q)
    try:
        assert names == rnames == en == qn
        assert list(cov.lens) == list(ref.lens) == [len(x) for x in ed] == [len(x) for x in eq]
        assert ncl == rncl == ecl_t + ecl_q
        sums = acc.cov_prepare(cov, 50, 7)
        assert sums == acc.cov_prepare(ref, 50, 7)
        assert sums == (sum(int(x.astype(np.int64).sum()) for x in ed), sum(int(x.astype(np.int64).sum()) for x in eq), sum(len(x) for x in ed))
        for c in range(len(names)):
            d, m = acc.cov_download(cov, c)
            rd, rm = acc.cov_download(ref, c)
            assert np.array_equal(d, ed[c]) and np.array_equal(m, eq[c]), (c, np.flatnonzero(d != ed[c])[:5], np.flatnonzero(m != eq[c])[:5])
            assert np.array_equal(rd, ed[c]) and np.array_equal(rm, eq[c])
        return [acc.cov_download(cov, c) for c in range(len(names))]
    finally:
        cov.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_abi_parity_at_the_tile_seams(acc, shape):
    contigs = SHAPES[shape]
    t = text_of(contigs)
    q = text_of(recut(contigs, 37 if shape != "one_position" else 1))      # the other file: the same contigs, other run boundaries
    check_parity(acc, t, q)
    check_parity(acc, q, t)


def test_feed_splits_do_not_matter(acc):
    """~40 records fed in pieces of 1, 2, 3, 7 and 64 bytes and as one piece — cuts inside a name, inside a number, between records, feeds
    without a whole record — the two files taking turns and one after the other: the same arrays every time"""
    rng = np.random.default_rng(5)
    contigs = [[(int(rng.integers(1, 400)), int(rng.choice([0, 3, 12, 65535, 70000, 123456]))) for _ in range(int(rng.integers(4, 10)))] for _ in range(6)]
    t = text_of(contigs, prefix=b"contig_name_")
    q = text_of(recut(contigs, 111), prefix=b"contig_name_").replace(b"\t", b"  ").replace(b"\n", b" \n\n", 3)
    assert 35 <= len(parse(t)) <= 70
    first = None
    for size in (None, 64, 7, 3, 2, 1):
        for alternate in (True, False):
            cut = (lambda x: [x]) if size is None else (lambda x: [x[i:i + size] for i in range(0, len(x), size)])
            got = check_parity(acc, t, q, pieces=(cut(t), cut(q)), alternate=alternate)
            if first is None:
                first = got
            for (d, m), (d0, m0) in zip(got, first):
                assert np.array_equal(d, d0) and np.array_equal(m, m0)


@pytest.mark.parametrize("at", [4095, 4096])
def test_token_at_a_tile_seam_of_the_tokeniser(acc, at):
    """one feed in which a token starts at the last byte of a tile of the tokeniser (4096 bytes) and at the first byte of the next one,
    behind a run of spaces"""
    contigs = [[(1 + i % 5, (7 * i) % 60) for i in range(130)] for _ in range(3)]
    t = token_at(text_of(contigs, prefix=b"contig_"), at)
    assert len(t) > at + 100
    check_parity(acc, t, text_of(recut(contigs, 37), prefix=b"contig_"))


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_records_at_the_tile_seam_of_the_offset_scan(acc, n):
    """one feed of exactly n fresh records: one tile of the 64-bit scan of the run lengths less one record, a whole tile, one record more"""
    contigs = [[(1 + i % 3, i % 50) for i in range(n)]]
    t = text_of(contigs)
    assert len(parse(t)) == n
    check_parity(acc, t, text_of(recut(contigs, 37)))


@pytest.mark.parametrize("head", [1, 7, 9])
def test_span_that_starts_off_a_16_byte_boundary(acc, head):
    """the first feed describes `head` positions: the next span starts at element `head` of the flat array, so its first lanes and its last
    ones store by element and every tile edge moves"""
    contigs = [[(head, 5), (T - head - 1, 6), (3, 7), (2 * T, 8)], [(T + 3, 9)]]
    t = text_of(contigs)
    q = text_of(recut(contigs, head))
    cut_t = t.index(b"\n") + 1
    cut_q = q.index(b"\n") + 1
    for alternate in (True, False):
        check_parity(acc, t, q, pieces=([t[:cut_t], t[cut_t:cut_t + 20], t[cut_t + 20:]], [q[:cut_q], q[cut_q:]]), alternate=alternate)


GOOD = [(b"c1", 0, 40, 5), (b"c1", 40, 90, 7), (b"c2", 0, 3, 70000), (b"c2", 3, 200, 1)]


def ingest_error(acc, t, q, **kw):
    t = t if isinstance(t, bytes) else fmt(t)
    q = q if isinstance(q, bytes) else fmt(q)
    with pytest.raises(BedgraphFormatError) as ei:
        acc.bedgraph_runs_ingest(kw.pop("tp", [t]), kw.pop("qp", [q]), **kw)[0].close()
    e = ei.value
    return (e.kind, e.file, e.record, e.a, e.b)


def swap(i, rec):
    return GOOD[:i] + [rec] + GOOD[i + 1:]


def test_every_check_through_the_abi(acc):
    assert ingest_error(acc, b"track type=bedGraph\n" + fmt(GOOD), GOOD) == (1, 0, 0, 1, 0)
    assert ingest_error(acc, GOOD, fmt(GOOD[:2]) + b"c2\t0\t3\t1.5\n") == (2, 1, 2, 3, 0)
    assert ingest_error(acc, GOOD, fmt(GOOD) + b"c3 0") == (2, 1, 4, 2, 0)                 # tokens left at the end of a file
    assert ingest_error(acc, fmt(GOOD) + b"c3 x 1", GOOD) == (1, 0, 4, 1, 0)
    assert ingest_error(acc, swap(2, (b"c2", 1, 3, 9)), GOOD) == (6, 0, 2, 1, 0)
    assert ingest_error(acc, GOOD, swap(1, (b"c1", 50, 90, 7))) == (7, 1, 1, 40, 50)       # a gap
    assert ingest_error(acc, swap(1, (b"c1", 30, 90, 7)), GOOD) == (7, 0, 1, 40, 30)       # an overlap
    assert ingest_error(acc, swap(3, (b"c2", 3, 3, 1)), GOOD) == (8, 0, 3, 3, 3)
    assert ingest_error(acc, GOOD, swap(0, (b"c1", 0, 40, -2))) == (9, 1, 0, -2, 0)
    # at finish: contig count, name, length
    assert ingest_error(acc, GOOD, GOOD[:2]) == (10, 0, 1, 200, 0)
    assert ingest_error(acc, GOOD[:2], GOOD) == (10, 0, 1, 0, 200)
    assert ingest_error(acc, GOOD, GOOD[:2] + [(b"cX", 0, 200, 1)]) == (10, 0, 1, 200, 200)
    assert ingest_error(acc, GOOD, swap(1, (b"c1", 40, 91, 7))) == (10, 0, 0, 90, 91)
    # no record at all in either file: a coverage without contigs, as from empty per-base files
    cov, names, ncl = acc.bedgraph_runs_ingest([b""], [b" \n"])
    assert (list(cov.lens), names, ncl) == ([], [], 0)
    cov.close()


def test_the_smallest_record_decides(acc):
    """two errors in one feed, hundreds of records apart (other workgroups of the record kernel) and next to each other; and in separate feeds"""
    runs = [(b"c", i * 3, i * 3 + 3, i % 9) for i in range(900)]
    bad = list(runs)
    bad[700] = (b"c", 2100, 2100, 1)          # kind 8 at record 700 (and record 701 still starts at the old end: no kind 7 there)
    bad[40] = (b"c", 121, 123, -5)            # kind 7 at record 40 (its negative value comes later in the order of the checks)
    assert ingest_error(acc, bad, runs) == (7, 0, 40, 120, 121)
    assert ingest_error(acc, runs, bad) == (7, 1, 40, 120, 121)
    bad2 = list(runs)
    bad2[41] = (b"c", 123, 126, -1)
    bad2[42] = (b"d", 4, 6, 1)
    assert ingest_error(acc, bad2, runs) == (9, 0, 41, -1, 0)
    text = fmt(bad)
    half = text.index(b"c\t1500\t")
    assert ingest_error(acc, text, runs, tp=[text[:half], text[half:]], qp=[fmt(runs)]) == (7, 0, 40, 120, 121)
    # the handle is as good as new for the next ingest
    check_parity(acc, fmt(runs), fmt(GOOD[:0] + [(b"c", 0, 2700, 3)]))


# ---- the CLI on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def run(cli, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def fixtures(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("runs_gpu")
    out = {"base": {}, "max": {}, "cut": {}}
    for k, fn in enumerate(("cov-total.bg", "cov-mq20.bg", "sparse-total.bg", "sparse-mq20.bg")):
        text = gzip.open(os.path.join(golden_dir, fn + ".gz")).read()
        for mode in out:
            p = d / (mode + "." + fn)
            p.write_bytes(text if mode == "base" else to_runs(text, mode, seed=100 + k))
            out[mode][fn] = str(p)
    return out


@pytest.mark.parametrize("args,exp", PANEL)
def test_cli_goldens_from_run_length_files(cli, golden_dir, fixtures, args, exp):
    a = panel_argv(fixtures["max"], args)
    rc, out, err = run(cli, a[:1] + ["--runs"] + a[1:])
    assert rc == 0, err.decode()
    assert out == golden(golden_dir, exp)


@pytest.mark.parametrize("args,exp", PANEL_ABORT)
def test_cli_aborts_from_run_length_files(cli, golden_dir, fixtures, args, exp):
    a = panel_argv(fixtures["cut"], args)
    rc, out, err = run(cli, a[:1] + ["--runs"] + a[1:])
    assert rc == -6, (rc, err.decode())
    assert out == golden(golden_dir, exp) == b""


@pytest.mark.parametrize("env", [{"CORNETTO_BG_PIECE": "32768"}, {"CORNETTO_BG_PIECE": "4000", "CORNETTO_DEVICES": "0,0"}])
def test_cli_in_dozens_of_feeds(cli, golden_dir, fixtures, env):
    """pieces of 32 KB (dozens of feeds per file; the cuts fall anywhere in a record), and pieces of 4000 bytes with the contigs dealt to
    two handles behind the ingest"""
    for args, exp in (PANEL[4], PANEL[10]):
        a = panel_argv(fixtures["cut"], args)
        rc, out, err = run(cli, a[:1] + ["--runs"] + a[1:], env)
        assert rc == 0, err.decode()
        assert out == golden(golden_dir, exp)


def test_cli_panel_option_and_errors(cli, fixtures, tmp_path):
    lens = {}
    for name, s, e, v in parse(open(fixtures["max"]["cov-total.bg"], "rb").read()):
        lens[name] = e
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, l) for n, l in lens.items()))
    opts = ["-w", "1000", "-i", "100", "-e", "2000", "-m", "10000", "--panel", str(tmp_path / "asm.bed"), "--panel-params", "300,2000,500,700,3000,2500,4000"]
    rc0, out0, err0 = run(cli, ["noboringbits", fixtures["base"]["cov-total.bg"], "-q", fixtures["base"]["cov-mq20.bg"]] + opts)
    assert rc0 == 0 and out0, err0.decode()
    rc, out, err = run(cli, ["noboringbits", "--runs", fixtures["cut"]["cov-total.bg"], "-q", fixtures["max"]["cov-mq20.bg"]] + opts)
    assert (rc, out) == (rc0, out0), err.decode()
    # a format error: one error line with the file and the record, exit 1, nothing on stdout; without --runs the file is refused as ever
    (tmp_path / "gap.bg").write_bytes(fmt(swap(1, (b"c1", 50, 90, 7))))
    (tmp_path / "ok.bg").write_bytes(fmt(GOOD))
    rc, out, err = run(cli, ["noboringbits", "--runs", str(tmp_path / "ok.bg"), "-q", str(tmp_path / "gap.bg")])
    assert rc == 1 and out == b"" and b"gap.bg: record 1:" in err and b"Found end 40, then start 50" in err and b"-bga" in err
    rc, out, err = run(cli, ["noboringbits", str(tmp_path / "ok.bg"), "-q", str(tmp_path / "ok.bg")])
    assert rc == 1 and out == b"" and b"end=start+1" in err
    (tmp_path / "empty.bg").write_bytes(b"")
    rc, out, err = run(cli, ["noboringbits", "--runs", str(tmp_path / "empty.bg"), "-q", str(tmp_path / "empty.bg")])
    assert rc == 0 and out == b"" and b"Number of contigs: 0" in err
