"""CPU: `seq -q FLOAT` on every host path — the kseq loop of `seq FILE`, --accel=no for --fastq and --bam (plain and under --bgzf) — with the
product binary and the sanitized build of the same host C, against tests/qmean_cases.py; the weight table of the header against `decimal`;
the chunk / range / lane-mask arithmetic of the kernel (csrc/qmean.hpp) as a CPU program under the host sanitizers; the usage errors and the
help line.  The device path is tests/test_gpu_qmean.py's.  Every test here fails on the parent commit: it has no -q and none of the symbols."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

import bgzf_cases as bc
import cornetto_amd
import qmean_cases as qc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = {"lane": qc.lane_seam_text, "chunk": qc.chunk_seam_text, "dense": qc.dense_text, "odd": qc.odd_text, "odd_crlf": lambda: qc.odd_text(True),
         "odd_no_newline": lambda: qc.odd_text(False, False), "boundary": qc.boundary_text, "window": qc.window_text, "wrapped": lambda: qc.wrapped_text()[0]}


def test_the_table(golden_dir):
    """the literal table of the header, entry by entry, and the six values the rule quotes"""
    assert [qc.E[q] for q in (0, 1, 10, 20, 30, 93)] == [1000000000, 794328235, 100000000, 10000000, 1000000, 1]
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    assert [int(L.cornetto_qual_weight(q)) for q in range(94)] == qc.E
    assert int(L.cornetto_qual_weight(-5)) == qc.E[0] and int(L.cornetto_qual_weight(94)) == int(L.cornetto_qual_weight(1000)) == qc.E[93] == 1
    assert qc.max_err(10) == 10 ** 8 and qc.max_err(0) == 10 ** 9 and qc.max_err(93) == 1 and qc.max_err(20) == 10 ** 7


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_fastq_host_paths(cli, tmp_path, name):        # noqa: F811
    text = TEXTS[name]()
    f = tmp_path / (name + ".fq")
    f.write_bytes(text)
    for m, t in ((0, 10), (20, 10), (0, 0), (0, 93), (0, 15.5)):
        w = qc.expect_fastq(text, m, qc.max_err(t))
        for args in ([str(f)], ["--accel=no", "--fastq", str(f)]):
            rc, out, err = run(cli, ["seq", "-m", str(m), "-q", str(t)] + args)
            assert rc == 0 and out == w.text and qc.summary_of(err) == qc.summary(w, m, t), (name, m, t, args)
    w = qc.expect_fastq(text, 0, qc.max_err(10))
    rc, out, err = run(cli, ["seq", "--accel=no", "-m", "0", "--min-qscore", "10", "--bgzf", "--fastq", str(f)])
    assert rc == 0 and out.endswith(bc.EOF_BLOCK) and gzip.decompress(out) == w.text and qc.summary_of(err) == qc.summary(w, 0, 10)
    w = qc.expect_fastq(text, 0, -1)          # without -q: no third line, the text of the length filter alone
    rc, out, err = run(cli, ["seq", "-m", "0", str(f)])
    assert rc == 0 and out == w.text and qc.summary_of(err) == qc.summary(w, 0) and b"mean qscore" not in err


def test_the_filter_drops_a_visible_share():
    for name in ("lane", "chunk", "window"):
        w = qc.expect_fastq(TEXTS[name](), 0, 10 ** 8)
        assert w.stats[2] // 4 < w.qstats[0] < 3 * w.stats[2] // 4, name


def test_a_fasta_record_passes(cli, tmp_path):        # noqa: F811
    """a record printed with an empty quality line passes (src/seq.c prints "(null)" for it only where printf does)"""
    f = tmp_path / "a.fa"
    f.write_bytes(b">a\nACGT\n>b c\nAC\nGT\n")
    rc0, ref, err0 = run(cli, ["seq", "-m", "0", str(f)])
    rc, out, err = run(cli, ["seq", "-m", "0", "-q", "93", str(f)])
    assert rc0 == rc == 0 and out == ref and b"mean qscore >= 93: 2\t8 bases" in err


def test_bam_host_path(cli, tmp_path):        # noqa: F811
    records = qc.bam_records()
    f = tmp_path / "r.bam"
    f.write_bytes(qc.bq.bam(records, [777] * 50))
    data = qc.bq.raw(records)
    for m, duplex, t in ((0, False, 10), (16, True, 10), (0, False, 0), (0, True, 93), (0, False, 7.25)):
        w = qc.expect_bam(data, m, duplex, qc.max_err(t))
        rc, out, err = run(cli, ["seq", "--accel=no", "-m", str(m), "-q", str(t), "--bam", str(f)] + (["--duplex"] if duplex else []))
        assert rc == 0 and out == w.text and qc.summary_of(err) == qc.summary(w, m, t), (m, duplex, t)
    w = qc.expect_bam(data, 0, False, qc.max_err(10))
    assert 5 < w.qstats[0] < w.stats[2] - 5
    rc, out, err = run(cli, ["seq", "--accel=no", "-m", "0", "-q", "10", "--bam", str(f), "--bgzf"])
    assert rc == 0 and gzip.decompress(out) == w.text and qc.summary_of(err) == qc.summary(w, 0, 10)
    # the pipe property on the host: the text of --bam through --fastq with -q is the text of --bam with -q
    rc, plain, err = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", str(f)])
    g = tmp_path / "piped.fq"
    g.write_bytes(plain)
    rc, out, err = run(cli, ["seq", "--accel=no", "-m", "0", "-q", "10", "--fastq", str(g)])
    assert rc == 0 and out == w.text and b"mean qscore" in err
    w0 = qc.expect_bam(data, 0, False, -1)
    assert plain == w0.text and qc.summary_of(run(cli, ["seq", "--accel=no", "-m", "0", "--bam", str(f)])[2]) == qc.summary(w0, 0)


def test_usage_errors_and_help(cli, tmp_path):        # noqa: F811
    f = tmp_path / "x.fq"
    f.write_bytes(b"@a\nAC\n+\nII\n")
    for bad in ("-1", "94", "x", "93.5", "1e", "nan", ""):
        for args in (["seq", "-q", bad, str(f)], ["seq", "--accel=no", "--min-qscore", bad, "--fastq", str(f)]):
            rc, out, err = run(cli, args)
            assert rc == 1 and out == b"" and b"total reads" not in err, args
            assert [ln for ln in err.split(b"\n") if ln.strip()] == [b"Error: min-qscore must be a number from 0 to 93"], err
    for ok in ("0", "93", "9.99", "1e1"):
        assert run(cli, ["seq", "-m", "0", "-q", ok, str(f)])[0] == 0
    rc, out, err = run(cli, ["seq", "-h"])
    lines = [ln for ln in out.split(b"\n") if b"-q FLOAT" in ln]
    assert rc == 0 and len(lines) == 1 and b"(not in the reference)" in lines[0] and b"--min-qscore" in lines[0]
    for word in (b"--bgzf", b"--fastq", b"--bam FILE", b"(extension)"):
        assert word not in lines[0]


def test_set_max_err_wants_an_object():
    """(after a feed: tests/test_gpu_qmean.py — an object needs a device)"""
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    assert L.cornetto_fqseq_set_max_err(None, None, 10 ** 8) == -3 and L.cornetto_bamfq_set_max_err(None, None, 10 ** 8) == -3
    p, n = C.c_void_p(), C.c_int64()
    assert L.cornetto_fqseq_qsums(None, None, C.byref(p), C.byref(n)) == -3 and L.cornetto_bamfq_qsums(None, None, C.byref(p), C.byref(n)) == -3
    qs = (C.c_int64 * 2)(7, 7)
    L.cornetto_fqseq_qstats(None, qs)
    L.cornetto_bamfq_qstats(None, qs)
    assert list(qs) == [7, 7]


# ---- the kernel's index arithmetic on the CPU, under the host sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/qmean_sim.cc: qm_first, qm_span, qm_lane and qm_weight (csrc/qmean.hpp) as qmean_sum calls them, the window and every table in a
    heap block of exactly its size, under AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("qmean_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "qmean_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "qmean_sim")

    def run_sim(window, ranges, bam=False):
        (d / "w.bin").write_bytes(window)
        (d / "r.txt").write_text("".join("%d %d\n" % r for r in ranges))
        r = subprocess.run([exe] + (["--bam"] if bam else []) + [str(d / "w.bin"), str(d / "r.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        return [int(x) for x in r.stdout.split()]
    return run_sim


def test_sim_fastq_cases(sim):
    for name in ("lane", "chunk", "dense", "odd", "odd_no_newline", "boundary", "window"):
        text = TEXTS[name]()
        ranges = qc.fastq_ranges(text)
        for m in (0, 20):          # a record -m drops is a range of length 0
            w = qc.expect_fastq(text, m, qc.ONE)
            assert sim(text, [(s, n if n >= m else 0) for s, n in ranges]) == w.sums, (name, m)
        for cut in (1, 15, 16, 17, 1023, 1024, 1025):          # the window ends inside a chunk, inside a lane's piece, inside a range
            if cut < len(text):
                short = text[:len(text) - cut]
                rs = [(s, max(0, min(n, len(short) - s))) for s, n in ranges if s <= len(short)]
                assert sim(short, rs) == [qc.qsum(short[s:s + n]) for s, n in rs], (name, cut)
    assert sim(b"", []) == [] and sim(b"IIII", []) == [] and sim(b"!", [(0, 1)]) == [qc.E[0]] and sim(b"!" * 5000, [(0, 0), (0, 5000), (5000, 0)]) == [0, 5000 * qc.E[0], 0]


def test_sim_bam_cases(sim):
    data = qc.bq.raw(qc.bam_records())
    ranges = qc.bam_ranges(data)
    raw_tab = [qc.E[min(c, 93)] for c in range(256)]
    assert sim(data, ranges, bam=True) == [sum(raw_tab[c] for c in data[s:s + n]) for s, n in ranges]
    w = qc.expect_bam(data, 0, False, qc.ONE)
    for (s, n), k, want in zip(ranges, w.keep, w.sums):
        if k >= 0 and n:          # (absent qualities are not summed: l_seq * E[1] takes the sum's place)
            assert sum(raw_tab[c] for c in data[s:s + n]) == want
