"""CPU: `cornetto qv -r` and `cornetto trioeval --pat-reads / --mat-reads` on the host path (--accel=no) with the product binary and the sanitized
build of the same host C, byte for byte against the formatter of tests/kcount_cases.py — stdout, -c, -b, --hist, the stderr line, the usage
errors, the overflow error — the statuses of the new entry points without their objects, and the arithmetic of the counted table (csrc/kqv.hpp)
as a CPU program under the host sanitizers.  The device path is tests/test_gpu_kcount.py's.  Every test here fails without the feature: the
options, the symbols and the sim do not exist."""
import gzip
import os
import subprocess

import pytest

import cornetto_amd
import kcount_cases as cc
import kqv_cases as kc
import ktrio_cases as kt
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def named(seqs, tag="c"):
    return [("%s%d" % (tag, i), s) for i, s in enumerate(seqs)]


def write_reads(d, case):
    """a file per batch, FASTQ and FASTA in turn (a record without bases goes into FASTA) -> [(channel, path, records)]"""
    out = []
    for i, (ch, seqs) in enumerate(case.reads):
        recs = named(seqs, "r%d_" % i)
        if i % 2 == 0 and all(len(s) for s in seqs):
            p = d / ("reads%d.fq" % i)
            p.write_bytes(cc.fastq(recs))
        else:
            p = d / ("reads%d.fa" % i)
            p.write_bytes(kc.fasta(recs, width=(0, 60, 7)[i % 3]))
        out.append((ch, str(p), recs))
    return out


def write_asm(d, query):
    q = named(query)
    (d / "asm.fa").write_bytes(kc.fasta(q, width=70))
    return str(d / "asm.fa"), q


def lines_of(err, tag):
    return [ln for ln in err.split(b"\n") if ln.startswith(tag)]


def qv_run(cli, d, k, files, m, apath, extra=()):        # noqa: F811
    args = ["qv", "--accel=no", "-k", str(k), "--min-count", str(m), "--hist", str(d / "h.tsv"), "-c", str(d / "c.tsv"), "-b", str(d / "b.bed")]
    for _, p, _ in files:
        args += ["-r", p]
    return run(cli, args + list(extra) + [apath])


def trio_run(cli, d, k, files, m, apath, extra=()):        # noqa: F811
    args = ["trioeval", "--accel=no", "-k", str(k), "--min-count", "%d,%d" % m, "--hist", str(d / "h.tsv"), "-c", str(d / "c.tsv")]
    for ch, p, _ in files:
        args += [("--pat-reads", "--mat-reads")[ch], p]
    return run(cli, args + list(extra) + [apath])


def test_the_restatement_agrees_with_the_sets_of_qv_and_trioeval():
    for k in cc.KS:
        e = cc.expected(k)
        for name, truth, query in kc.cases(k):
            S, n_pos = kc.truth_set([s for b in truth for s in b], k)
            case, st, hists, by_m = e["m1_identity/" + name]
            assert st == (n_pos, len(S)) and by_m[(1,)] == ((len(S),), kc.query(S, query, k)) and sum(hists[0]) == len(S), name
        batches, query, st, rows = kt.expected(k)["mosaic"]
        case, st2, hists, by_m = e["mosaic_twice"]
        assert st2 == (2 * st[0], st[1]) and by_m[(2, 2)][1] == rows and hists[0][1] == hists[1][1] == 0
        # the planted counts: every bin is exact, and the bins sum to distinct
        case, st, hists, by_m = e["hist_bins"]
        n = 40 - k + 1
        assert [hists[0][c] for c in (1, 2, 3, 4, 1021, 1022, 1023)] == [n, n, n, 0, 0, n, 2 * n] and sum(hists[0]) == st[1] == 6 * n and hists[0][0] == 0
        assert [by_m[m][0] for m in case.ms] == [(4 * n,), (2 * n,), (n,), (0,)]
        # one key above the cap: solid for m = 65535, in the last bin, the G/C key beside it
        case, st, hists, by_m = e["cap_and_last_bin"]
        assert st == (17 * cc.TILE - k + 1 + cc.TILE - k + 1, 2) and hists[0][1023] == 2 and sum(hists[0]) == 2
        assert [by_m[m][0] for m in case.ms] == [(1,), (2,), (1,), (2,)] and 17 * cc.TILE - k + 1 > cc.CAP
        # m = 2 drops the error k-mers of the short reads: fewer solid keys than distinct ones, and the clean sequence misses nearly nothing
        case, st, hists, by_m = e["short_reads"]
        assert by_m[(2,)][0][0] < by_m[(1,)][0][0] == st[1] and hists[0][1] > 0
        # the nine pairs of counts: with m = (2, 2) one marker of either type, with (1, 1) three of either
        case, st, hists, by_m = e["two_channels"]
        assert by_m[(2, 2)][0] == (3, 3) and by_m[(1, 1)][0] == (6, 6) and by_m[(1, 2)][0] == (6, 3)
        assert by_m[(2, 2)][1][0][1:3] == [2, 2] and by_m[(1, 1)][1][0][1:3] == [2, 2] and by_m[(1, 2)][1][0][1:3] == [4, 1]
        case, st, hists, by_m = e["multiplicity"]
        assert by_m[(1,)][0][0] > by_m[(2,)][0][0] > by_m[(3,)][0][0] and by_m[(1,)][1][1][0] == 0
        assert k == 11 or by_m[(3,)][0][0] == 0          # m = 3: every slot a tombstone (a random 11-mer recurs now and then)


@pytest.mark.parametrize("k", cc.KS)
def test_host_path_cases(cli, tmp_path, k):        # noqa: F811
    for name, (case, st, hists, by_m) in cc.expected(k).items():
        d = tmp_path / name.replace("/", "_")
        d.mkdir()
        files = write_reads(d, case)
        apath, q = write_asm(d, case.query)
        extra = ["--slots", str(cc.slots_of(case, st))] if case.slots else []
        for m in case.ms:
            if case.channels == 1:
                w = cc.expect_qv([r for _, _, r in files], [(apath, q)], k, m[0])
                rc, out, err = qv_run(cli, d, k, files, m[0], apath, extra)
                assert rc == 0 and out == w["stdout"], (name, m, err[-2000:])
                assert (d / "c.tsv").read_bytes() == w["contigs"] and (d / "b.bed").read_bytes() == w["bed"], (name, m)
                assert lines_of(err, b"[qv]") == [w["line"]], (name, m)
            else:
                w = cc.expect_trio([r for ch, _, r in files if ch == 0], [r for ch, _, r in files if ch == 1], [(apath, q)], k, m)
                rc, out, err = trio_run(cli, d, k, files, m, apath, extra)
                assert rc == 0 and out == w["stdout"], (name, m, err[-2000:])
                assert (d / "c.tsv").read_bytes() == w["contigs"] and lines_of(err, b"[trioeval]") == [w["line"]], (name, m)
            assert (d / "h.tsv").read_bytes() == w["hist"] and w["hist"].count(b"\n") == 1023, (name, m)


def test_min_count_1_prints_what_the_truth_assembly_prints(cli, tmp_path):        # noqa: F811
    k = 21
    cs = dict((n, (t, q)) for n, t, q in kc.cases(k))
    truth, query = cs["two_batches"]
    x = tmp_path / "x.fa"
    x.write_bytes(kc.fasta(named([s for b in truth for s in b], "t")))
    g = tmp_path / "x.fa.gz"
    g.write_bytes(gzip.compress(x.read_bytes()))
    apath, q = write_asm(tmp_path, query)
    rc0, out0, err0 = run(cli, ["qv", "--accel=no", str(x), apath])
    rc1, out1, err1 = run(cli, ["qv", "--accel=no", "-r", str(x), "--min-count", "1", apath])
    assert rc0 == rc1 == 0 and out0 == out1 and out0.count(b"\n") == 2
    # the default threshold is 2: every k-mer of the truth twice, from a plain and a gzip file, is the same set again; two assemblies in turn
    env = dict(os.environ, CORNETTO_ACCEL="no")
    p = subprocess.run([cli, "qv", "-r", str(x), "-r", str(g), apath, apath], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and p.stdout == out0 + out0.split(b"\n", 1)[1] and b"(count >= 2)" in lines_of(p.stderr, b"[qv]")[0]
    # the same for the parents of trioeval
    batches, query, st, rows = kt.expected(k)["mosaic"]
    pf, mf = tmp_path / "p.fa", tmp_path / "m.fa"
    pf.write_bytes(kc.fasta(named([s for t, b in batches if t == kt.PAT for s in b], "p")))
    mf.write_bytes(kc.fasta(named([s for t, b in batches if t == kt.MAT for s in b], "m")))
    apath, q = write_asm(tmp_path, query)
    rc0, out0, err0 = run(cli, ["trioeval", "--accel=no", str(pf), str(mf), apath])
    rc1, out1, err1 = run(cli, ["trioeval", "--accel=no", "--pat-reads", str(pf), "--mat-reads", str(mf), "--min-count", "1", apath])
    rc2, out2, err2 = run(cli, ["trioeval", "--accel=no", "--pat-reads", str(pf), "--pat-reads", str(pf), "--mat-reads", str(mf), "--min-count", "2,1", apath])
    assert rc0 == rc1 == rc2 == 0 and out0 == out1 == out2 and b"(count >= 2,1)" in lines_of(err2, b"[trioeval]")[0]


def test_overflow_and_table_sizes(cli, tmp_path):        # noqa: F811
    k = 21
    case, st, hists, by_m = cc.expected(k)["tombstones_at_load_1"]
    files = write_reads(tmp_path, case)
    apath, q = write_asm(tmp_path, case.query)
    for slots in (st[1] - 1, 1):
        rc, out, err = qv_run(cli, tmp_path, k, files, 2, apath, ["--slots", str(slots)])
        lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
        assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and b"overflowed" in lines[0] and not lines_of(err, b"[qv]"), (slots, err)
    case, st, hists, by_m = cc.expected(k)["two_channels"]
    files = write_reads(tmp_path, case)
    apath, q = write_asm(tmp_path, case.query)
    w = cc.expect_trio([r for ch, _, r in files if ch == 0], [r for ch, _, r in files if ch == 1], [(apath, q)], k, (2, 2))
    rc, out, err = trio_run(cli, tmp_path, k, files, (2, 2), apath, ["--slots", str(st[1])])          # load 1.0
    assert rc == 0 and out == w["stdout"] and lines_of(err, b"[trioeval]") == [w["line"]]
    rc, out, err = trio_run(cli, tmp_path, k, files, (2, 2), apath, ["--slots", str(st[1] - 1)])
    lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
    assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and b"overflowed" in lines[0]
    # a table that cannot be had: one ERROR line that names --slots, 12 bytes per slot for qv and 16 for trioeval
    if "asan" in os.path.basename(cli):          # (the sanitizer's allocator reports an impossible size itself instead of returning null)
        return
    big = 1 << 58
    rc, out, err = run(cli, ["qv", "--accel=no", "--slots", str(big), "-r", files[0][1], apath])
    lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
    assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and str(big * 12).encode() in lines[0]
    rc, out, err = run(cli, ["trioeval", "--accel=no", "--slots", str(big), "--pat-reads", files[0][1], "--mat-reads", files[1][1], apath])
    lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
    assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and str(big * 16).encode() in lines[0]


def test_usage_errors_and_help(cli, tmp_path):        # noqa: F811
    f = tmp_path / "t.fa"
    f.write_bytes(b">a\n" + b"ACGT" * 20 + b"\n")
    t, h = str(f), str(tmp_path / "h.tsv")
    bad = [["qv", "-r", t], ["qv", "-r", t, "-t", t, t], ["qv", "--min-count", "2", t, t], ["qv", "--hist", h, t, t], ["qv", "-r", t, "--min-count", "0", t],
           ["qv", "-r", t, "--min-count", "65536", t], ["qv", "-r", t, "--min-count", "2x", t], ["qv", "-r", t, "--min-count", "2,2", t], ["qv", "-r", t, "--min-count", "", t],
           ["qv", "-r", t, "-c", str(tmp_path / "c"), t, t], ["qv", "--accel=no", "-r", "-", t],
           ["trioeval", "--pat-reads", t, t], ["trioeval", "--mat-reads", t, t], ["trioeval", "--pat-reads", t, "--mat-reads", t],
           ["trioeval", "--pat-reads", t, "--mat-reads", t, "-P", t, t], ["trioeval", "--pat-reads", t, "--mat-reads", t, "-M", t, t],
           ["trioeval", "--min-count", "2", t, t, t], ["trioeval", "--hist", h, t, t, t], ["trioeval", "--pat-reads", t, "--mat-reads", t, "--min-count", "0", t],
           ["trioeval", "--pat-reads", t, "--mat-reads", t, "--min-count", "2,0", t], ["trioeval", "--pat-reads", t, "--mat-reads", t, "--min-count", "2,", t],
           ["trioeval", "--pat-reads", t, "--mat-reads", t, "--min-count", "1,2,3", t], ["trioeval", "--pat-reads", t, "--mat-reads", t, "--min-count", "65536", t],
           ["trioeval", "--accel=no", "--pat-reads", "-", "--mat-reads", t, t]]
    for args in bad:
        rc, out, err = run(cli, args)
        assert rc == 1 and out == b"" and not lines_of(err, b"[qv]") and not lines_of(err, b"[trioeval]") and not os.path.exists(h), args
    for cmd in ("qv", "trioeval"):
        rc, out, err = run(cli, [cmd, "-h"])
        assert rc == 0 and b"--min-count" in out and b"--hist" in out and b"1.5 times" in out
    rc, out, err = run(cli, ["qv", "--accel=no", "-r", t, "--min-count", "65535", t])
    assert rc == 0 and b"0 solid (count >= 65535)" in lines_of(err, b"[qv]")[0]


def test_the_entry_points_want_their_objects():
    import ctypes as C
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    p = C.c_void_p(7)
    assert L.cornetto_kset_open_counted(None, 21, 100, 1, C.byref(p)) == cc.E_ARG and L.cornetto_kset_open_counted(None, 21, 100, 3, C.byref(p)) == cc.E_ARG
    assert L.cornetto_kset_open_counted(None, 21, 100, 1, None) == cc.E_ARG
    assert L.cornetto_kset_count(None, None, None, 0) == cc.E_ARG
    hist = (C.c_int64 * cc.BINS)()
    assert L.cornetto_kset_hist(None, None, 0, hist) == cc.E_ARG
    m, solid = (C.c_int32 * 2)(1, 1), (C.c_int64 * 2)()
    assert L.cornetto_kset_seal(None, None, m, solid) == cc.E_ARG
    assert cornetto_amd.KSET_COUNT_CAP == cc.CAP and cornetto_amd.KSET_HIST_BINS == cc.BINS


# ---- the kernels' arithmetic on the CPU, under the host sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/kcount_sim.cc: the run-dealing, the count walk, the bins, the seal and the two lookups of csrc/kqv.hpp as the kernels call them;
    every record, the prefix, the table, the counts and the histogram in a heap block of exactly its size, under AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("kcount_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "kcount_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "kcount_sim")

    def batch(seqs):
        return b"%d\n" % len(seqs) + b"".join(b"%d\n" % len(s) + s + b"\n" for s in seqs)

    def run_sim(k, slots, case, m):
        mm = tuple(m) + (1,) * (2 - len(m))
        (d / "case.bin").write_bytes(b"%d %d %d %d\n" % (k, slots, case.channels, len(case.reads)) + b"".join(b"%d\n" % ch + batch(b) for ch, b in case.reads) +
                                     b"%d %d\n" % mm + batch(case.query))
        r = subprocess.run([exe, str(d / "case.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln]
        if lines[0] == ["overflow"]:
            return None
        hists = [[0] * cc.BINS for _ in range(case.channels)]
        for ln in lines:
            if ln[0] == "h":
                hists[int(ln[1])][int(ln[2])] = int(ln[3])
        st = tuple(map(int, lines[0][1:]))
        solid = tuple(map(int, next(ln for ln in lines if ln[0] == "solid")[1:]))
        if case.channels == 1:
            cs = [tuple(map(int, ln[1:])) for ln in lines if ln[0] == "c"]
            return st, hists, solid, ([c[0] for c in cs], [c[1] for c in cs])
        return st, hists, solid, [list(map(int, ln[1:])) for ln in lines if ln[0] == "t"]
    return run_sim


@pytest.mark.parametrize("k", cc.KS)
def test_sim_cases(sim, k):
    for name, (case, st, hists, by_m) in cc.expected(k).items():
        for m in case.ms:
            solid, res = by_m[m]
            want = (st, hists, solid, (res[0], res[1]) if case.channels == 1 else res)
            assert sim(k, cc.slots_of(case, st), case, m) == want, (name, m)
            if name in ("tombstones_at_load_1", "two_channels", "short_reads", "m1_identity/short_contigs", "m1_identity/two_batches"):
                assert sim(k, st[1], case, m) == want, (name, m)                  # load 1.0
                assert sim(k, st[1] - 1, case, m) is None, (name, m)              # a table that is too small is a status
                assert sim(k, 1, case, m) is None, (name, m)
