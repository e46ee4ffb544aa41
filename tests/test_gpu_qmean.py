"""GPU: `seq -q`, the mean-quality filter summed on the device (csrc/qmean.hip: qmean_sum; fqseq.hip, bamfq.hip; Accel.fastq_seq / bam_fastq with
max_err; the CLI), against tests/qmean_cases.py with exact equality: the text, the four counts of the two summary lines, the printed reads and
bases, the keep column of the record table and every record's sum.  The index arithmetic of the cases went through tools/sim/qmean_sim.cc
under the host sanitizers first (tests/test_qmean_host.py).  Every test here fails on the parent commit: it has no max_err."""
import gzip
import subprocess

import pytest

import bgzf_cases as bc
import cornetto_amd
import qmean_cases as qc

pytestmark = pytest.mark.gpu
Q10 = 10 ** 8
THRESHOLDS = (-1, 0, qc.ONE, 31622777)          # off, nothing but error-free reads, everything, Q15


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def check_fastq(acc, text, m, p, what=None, part=None, data=None, **kw):
    """one run against the expectation; part: the device's part of the text ends there (the rest is the sequential reader's); data: the text
    as it is fed (a BGZF blob)"""
    out, stats, recs, rest, plain = acc.fastq_seq(text if data is None else data, m, max_err=None if p < 0 else p, **kw)
    w = qc.expect_fastq(text if part is None else text[:part], m, p)
    if kw.get("bgzf_out"):
        out = gzip.decompress(b"".join(out)) if out else b""
    assert rest == (len(text) if part is None else part) and plain == (part is None), (what, rest, plain)
    assert out == w.text, (what, len(out), len(w.text))
    assert stats == w.stats and acc.fq_qstats == (w.qstats if p >= 0 else w.stats[2:]), (what, stats, acc.fq_qstats, w.stats, w.qstats)
    assert [int(k) for k in recs["keep"]] == w.keep, what
    if p >= 0:
        assert [int(s) for s in acc.fq_qsums] == w.sums, what
    else:
        assert acc.fq_qsums is None
    return w


def check_bam(acc, records, m, duplex, p, what=None, sizes=None, **kw):
    blob = qc.bq.bam(records, sizes)
    out, stats, recs = acc.bam_fastq(blob, m, duplex, max_err=None if p < 0 else p, **kw)
    w = qc.expect_bam(qc.bq.raw(records), m, duplex, p)
    assert out == w.text, (what, len(out), len(w.text))
    assert stats == w.stats and acc.bam_qstats == (w.qstats if p >= 0 else w.stats[2:]), (what, stats, acc.bam_qstats, w.stats, w.qstats)
    assert [int(k) for k in recs["kept"]] == w.keep, what
    if p >= 0:
        assert [int(s) for s in acc.bam_qsums] == w.sums, what
    return w


def test_the_table_is_the_librarys(acc):
    assert [int(acc.L.cornetto_qual_weight(q)) for q in range(94)] == qc.E
    assert all(qc.E[q] == v for q, v in qc.KNOWN.items())


def test_lane_seams(acc):
    """the quality line at every offset modulo 16 with every length 1 .. 48"""
    text = qc.lane_seam_text()
    w = check_fastq(acc, text, 0, Q10)
    assert 200 < w.qstats[0] < len(w.keep) - 200          # the filter drops a visible share
    check_fastq(acc, text, 20, Q10)


def test_chunk_and_workgroup_seams(acc):
    """lines across the 1 KiB and 4 KiB multiples of the window, lines over three and more chunks"""
    text = qc.chunk_seam_text()
    for off, n in qc.fastq_ranges(text):
        assert n < 100 or off // qc.CHUNK + 2 <= (off + n - 1) // qc.CHUNK
    w = check_fastq(acc, text, 0, Q10)
    assert 10 < w.qstats[0] < len(w.keep) - 10
    check_fastq(acc, text, 0, Q10, window=len(text) // 2 + 7)          # the same lines at other places of the window


def test_dense_chunk(acc):
    text = qc.dense_text()
    assert min(sum(1 for off, n in qc.fastq_ranges(text) if off // qc.CHUNK == c) for c in (0, 1)) > 64
    w = check_fastq(acc, text, 0, Q10)
    assert w.qstats == [200, 200]


def test_odd_records(acc):
    for crlf in (False, True):
        for last_newline in (True, False):
            text = qc.odd_text(crlf, last_newline)
            for p in (Q10, 0, qc.ONE, 10 ** 9 // 2):
                check_fastq(acc, text, 0, p, (crlf, last_newline, p))
    w = qc.expect_fastq(qc.odd_text(), 0, Q10)
    assert w.sums[1] == 5 * qc.E[0] and w.sums[2] == 5 * qc.E[93] and w.keep[:4] == [1, 0, 1, 1]          # clamped below '!' and above '~'; L = 0 passes
    assert w.keep[5:7] == [1, 0]                                                                          # all Q10, and one Q9 among them


def test_boundary_of_the_rule(acc):
    text = qc.boundary_text()
    w = check_fastq(acc, text, 0, Q10)
    assert w.keep[:10] == [1] * 10 and w.sums[18] == 7 * 10 ** 13 and w.keep[18] == 0          # equality keeps; above 2^32 by far
    w = check_fastq(acc, text, 0, Q10 - 1)
    assert w.keep[:10] == [0] * 10
    assert w.keep[10:18] == [0, 0, 0, 0, 1, 1, 1, 1]          # one Q0 among n Q40s, n = 1, 2, 9, 10, 11, ..: 10^9 + (n - 1) 10^5 <= (10^8 - 1) n from n = 11 on
    check_fastq(acc, text, 1000, Q10)


def test_several_windows_on_one_object(acc):
    """nothing survives from the last window: every record is summed once, in the window that holds it whole"""
    text = qc.window_text()
    least = qc.longest_record(text)
    for window, slab, feeds in ((least, 64, 3), (1000, 300, 3), (2 * least + 17, None, 3), (4096, 100, 1)):
        w = check_fastq(acc, text, 0, Q10, (window, slab, feeds), window=window, slab=slab, feeds=feeds)
    assert 20 < w.qstats[0] <= 100


def test_randomised_run(acc):
    text = qc.random_text()
    w = check_fastq(acc, text, 0, 31622777, window=65536)
    assert 200 < w.qstats[0] < 1800
    check_fastq(acc, text, 2500, 31622777, window=65536, feeds=3)


@pytest.mark.parametrize("p", THRESHOLDS)
def test_thresholds_and_options(acc, p):
    text = qc.window_text()
    for m in (0, 150):
        check_fastq(acc, text, m, p, ("min_len", m))
    blob = bc.write(text, [1000] * (len(text) // 1000 + 1))
    check_fastq(acc, text, 100, p, "bgzf_in", data=blob, bgzf_in=True, window=qc.longest_record(text) + 1000)
    check_fastq(acc, text, 100, p, "bgzf_out", bgzf_out=True, window=4096, slab=1000)
    text, at = qc.wrapped_text()
    check_fastq(acc, text, 0, p, "wrapped", part=at)


def test_set_max_err_is_checked(acc):
    import ctypes as C
    L = acc.L
    opt = cornetto_amd.FqSeqOpt()
    L.cornetto_fqseq_defaults(C.byref(opt))
    opt.window = 4096
    fq = C.c_void_p()
    assert L.cornetto_fqseq_open(acc.h, C.byref(opt), C.byref(fq)) == 0
    try:
        assert L.cornetto_fqseq_set_max_err(acc.h, fq, -2) == -3 and L.cornetto_fqseq_set_max_err(acc.h, fq, qc.ONE + 1) == -3
        assert L.cornetto_fqseq_set_max_err(acc.h, fq, qc.ONE) == 0 and L.cornetto_fqseq_set_max_err(acc.h, fq, -1) == 0
        t = b"@a\nAC\n+\nII\n"
        src = cornetto_amd.BgSrc(t, len(t), None, None, 0)
        taken, n_text, pl = C.c_int64(), C.c_int64(), C.c_int32()
        assert L.cornetto_fqseq_feed(acc.h, fq, C.byref(src), 1, C.byref(taken), C.byref(n_text), C.byref(pl)) == 0
        assert L.cornetto_fqseq_set_max_err(acc.h, fq, Q10) == -3          # after a feed
        p, n = C.c_void_p(), C.c_int64()
        assert L.cornetto_fqseq_qsums(acc.h, fq, C.byref(p), C.byref(n)) == -3          # no filter, no record table: no sums
    finally:
        L.cornetto_fqseq_close(acc.h, fq)


# ---- BAM ----------------------------------------------------------------------------------------------------------------------------------------
def test_bam_records(acc):
    """reverse strand, absent qualities, raw qualities above 93, odd l_seq, long names and CIGARs, auxiliary fields behind the qualities,
    SECONDARY records, --duplex with the threshold"""
    records = qc.bam_records()
    for p in THRESHOLDS + (Q10,):
        for m, duplex in ((0, False), (16, True)):
            w = check_bam(acc, records, m, duplex, p, (p, m, duplex))
    w = qc.expect_bam(qc.bq.raw(records), 0, False, Q10)
    assert w.sums[60] == 35 * qc.E[1] and w.sums[61] == 1005 * qc.E[1] and w.keep[60:62] == [0, 0]          # absent: '"' each
    assert w.sums[62] == 164 * qc.E[93] and w.sums[63] == 161 * qc.E[93] + 3 * qc.E[0]                      # raw 94 .. 254 print as '~'
    assert w.keep[65:67] == [-1, -1] and w.sums[65:67] == [0, 0] and w.keep[67] == 1                        # passed over; all Q10: equality
    assert 5 < w.qstats[0] < 60


def test_bam_across_blocks_and_windows(acc):
    records = qc.bam_records()
    data = qc.bq.raw(records)
    least = max(n for _, n in qc.bam_cases.record_sizes(data))
    sizes = [777] * (len(data) // 777)
    for window, slab, feeds in ((least + 777, 4096, 3), (2 * least + 1000, None, 2)):
        check_bam(acc, records, 0, False, Q10, (window, slab, feeds), sizes=sizes, window=window, slab=slab, feeds=feeds)
        check_bam(acc, records, 16, True, Q10, (window, slab, feeds), sizes=sizes, window=window, slab=slab, feeds=feeds)


def test_bam_pipe_property(acc):
    """seq --bam F -q T prints what seq --bam F -m .. | seq --fastq - -m 0 -q T prints"""
    blob = qc.bq.bam(qc.bam_records())
    for m in (0, 17):
        for p in (Q10, 31622777, 0):
            text = acc.bam_fastq(blob, m)[0]
            want = acc.fastq_seq(text, 0, max_err=p)[0]
            got = acc.bam_fastq(blob, m, max_err=p)
            assert got[0] == want and acc.bam_qstats == acc.fq_qstats
            assert [int(s) for s, k in zip(acc.bam_qsums, got[2]["kept"]) if k >= 0 and int(s)] == [int(s) for s in acc.fq_qsums if int(s)]


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------------
def _cli(args):
    p = subprocess.run([cornetto_amd.CLI_PATH, "seq"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, qc.summary_of(p.stderr)


def test_cli(tmp_path):
    text = qc.window_text() + qc.odd_text()
    fq, bam = tmp_path / "r.fq", tmp_path / "r.bam"
    fq.write_bytes(text)
    records = qc.bam_records()
    bam.write_bytes(qc.bq.bam(records))
    for m in (0, 100):
        w = qc.expect_fastq(text, m, qc.max_err(10))
        assert 0 < w.qstats[0] < w.stats[2]
        for args in (["--fastq", str(fq)], ["--accel=no", "--fastq", str(fq)], [str(fq)], ["--accel=no", str(fq)]):
            assert _cli(["-m", str(m), "-q", "10"] + args) == (w.text, qc.summary(w, m, 10)), (m, args)
            assert _cli(["-m", str(m), "--min-qscore", "10"] + args) == (w.text, qc.summary(w, m, 10)), (m, args)
        w = qc.expect_bam(qc.bq.raw(records), m, False, qc.max_err(10))
        for args in (["--bam", str(bam)], ["--accel=no", "--bam", str(bam)]):
            assert _cli(["-m", str(m), "-q", "10"] + args) == (w.text, qc.summary(w, m, 10)), (m, args)
        out, err = _cli(["-m", str(m), "-q", "10", "--bam", str(bam), "--bgzf"])
        assert gzip.decompress(out) == w.text and err == qc.summary(w, m, 10)
    # a fraction of a score; and without -q no third line
    w = qc.expect_fastq(text, 0, qc.max_err(12.5))
    assert _cli(["-m", "0", "-q", "12.5", "--fastq", str(fq)]) == (w.text, qc.summary(w, 0, 12.5))
    w = qc.expect_fastq(text, 0, -1)
    assert _cli(["-m", "0", "--fastq", str(fq)]) == (w.text, qc.summary(w, 0)) and b"mean qscore" not in _cli(["-m", "0", "--bam", str(bam)])[1]
