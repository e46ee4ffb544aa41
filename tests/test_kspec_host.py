"""CPU: `cornetto qv -r ... --completeness --spectra-cn FILE` on the host path (--accel=no) with the product binary and the sanitized build of the same
host C, byte for byte against the texts of tests/kspec_cases.py — stdout with the three columns, the spectrum file, the usage errors, the overflow
error — the statuses of the new entry points without their objects, and the arithmetic of the copies and the spectrum (csrc/kqv.hpp) as a CPU
program under the host sanitizers.  The device path is tests/test_gpu_kspec.py's.  Every test but the check of the restatement and the guard fails without the feature:
the options, the symbols and the sim do not exist."""
import functools
import os
import subprocess

import pytest

import cornetto_amd
import kcount_cases as cc
import kqv_cases as kc
import kspec_cases as ks
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def named(seqs, tag="c"):
    return [("%s%d" % (tag, i), s) for i, s in enumerate(seqs)]


def lines_of(err, tag):
    return [ln for ln in err.split(b"\n") if ln.startswith(tag)]


@functools.lru_cache(maxsize=None)
def expect(k, name, m):
    """the texts of a case with its assembly given as `asm.fa` (the runs' working directory holds it): once per case, for both builds of the CLI"""
    c = ks.expected(k)[name].case
    return ks.expect_qv([named(seqs, "r%d_" % i) for i, seqs in enumerate(c.reads)], [("asm.fa", named([s for b in c.asm for s in b]))], k, m)


def write_case(d, case):
    """a -r file per batch of reads (FASTQ; FASTA where a record has no bases) and the assembly's batches in one file -> (read files, path, contigs)"""
    files = []
    for i, seqs in enumerate(case.reads):
        recs = named(seqs, "r%d_" % i)
        p = d / ("reads%d.%s" % (i, "fq" if all(len(s) for s in seqs) else "fa"))
        p.write_bytes(cc.fastq(recs) if p.suffix == ".fq" else kc.fasta(recs))
        files.append((str(p), recs))
    q = named([s for b in case.asm for s in b])
    (d / "asm.fa").write_bytes(kc.fasta(q, width=70))
    return files, str(d / "asm.fa"), q


def qv_args(k, m, files, extra=()):
    args = ["qv", "--accel=no", "-k", str(k), "--min-count", str(m)]
    for p, _ in files:
        args += ["-r", p]
    return args + list(extra)


def test_the_restatement_on_the_planted_counts():
    """the Python restatement alone: that the cases reach the count and copy classes they are built for.  It runs no code of the feature and
    passes without it, like the guard at the end"""
    for k in ks.KS:
        e = ks.expected(k)
        p = e["planted"]
        reads, contigs, plan = ks.planted(__import__("random").Random(4000 + k))
        n = 40 - k + 1
        want = [[0] * ks.BINS for _ in range(ks.CN)]
        for c, a in plan:
            if c or a:
                want[min(a, 5)][min(c, 1023)] += n
        assert p.spec == want and p.spec[0][0] == 0
        # every count class meets several copy classes, and count 0 meets copies >= 1: row 0 is the assembly-only keys
        for c in (0, 1, 2, 3, 1022, 1023):
            assert sum(1 for a in range(ks.CN) if p.spec[a][c]) >= 2, (k, c)
        assert sum(p.spec[a][0] for a in range(1, ks.CN)) > 0
        assert all(sum(p.spec[a][c] for a in range(ks.CN)) == p.hist[c] for c in range(1, ks.BINS))
        # solid and found where the bins cannot give them: the units counted 1023 and 1024 times share the last bin
        solid = dict((m, sum(n for c, a in plan if c >= m)) for m in ks.PLANTED_MS)
        found = dict((m, sum(n for c, a in plan if c >= m and a)) for m in ks.PLANTED_MS)
        assert p.totals == dict((m, (solid[m], found[m])) for m in ks.PLANTED_MS)
        assert p.totals[1024] != p.totals[1023] and p.totals[1025] == (0, 0) and 0 < p.totals[1][1] < p.totals[1][0]
        # the order and the batches of the contigs change nothing
        assert e["batches/two"].spec == e["batches/reversed"].spec == p.spec and e["batches/two"].totals == p.totals
        one = e["one_key"]
        assert one.spec[5][100 - k + 1] == 1 and sum(map(sum, one.spec)) == 1 and one.totals[1] == (1, 1) and one.totals[100 - k + 2] == (0, 0)
        nb = e["neighbours_at_load_1"]
        assert sum(nb.spec[a][0] for a in range(ks.CN)) == nb.union - nb.stats[1] > 0
        assert ks.completeness(0, 0) == "NA" and ks.completeness(3, 2) == "0.666667"


@pytest.mark.parametrize("k", ks.KS)
def test_host_path_cases(cli, tmp_path, k):        # noqa: F811
    for name, e in ks.expected(k).items():
        if name.startswith("batches/"):          # (a file is batched by the streamer, not by the caller)
            continue
        d = tmp_path / name.replace("/", "_")
        d.mkdir()
        files, _, q = write_case(d, e.case)
        apath = "asm.fa"
        extra = ["--slots", str(ks.slots_of(e))] if e.case.slots else []
        for m in e.case.ms[:3] + e.case.ms[4:5]:
            w = expect(k, name, m)
            rc, out, err = run(cli, qv_args(k, m, files, extra) + ["--completeness", "--spectra-cn", str(d / "s.tsv"), "--hist", str(d / "h.tsv"), apath], cwd=str(d))
            assert rc == 0 and out == w["stdout"], (name, m, err[-2000:])
            assert (d / "s.tsv").read_bytes() == w["spectra"] and w["spectra"].count(b"\n") == 1025, (name, m)
            assert (d / "h.tsv").read_bytes() == w["hist"] and lines_of(err, b"[qv]") == [w["line"]], (name, m)
            solid, found = e.totals[m]
            assert out.split(b"\n")[1].split(b"\t")[-3:] == [b"%d" % solid, b"%d" % found, ks.completeness(solid, found).encode()], (name, m)
        # either option alone, and neither: the bytes of today
        rc, out, err = run(cli, qv_args(k, m, files, extra) + ["--spectra-cn", str(d / "s2.tsv"), apath], cwd=str(d))
        assert rc == 0 and out == w["plain"] and (d / "s2.tsv").read_bytes() == w["spectra"], name
        rc, out, err2 = run(cli, qv_args(k, m, files, extra) + [apath], cwd=str(d))
        assert rc == 0 and out == w["plain"] and lines_of(err2, b"[qv]") == lines_of(err, b"[qv]") == [w["line"]], name


def test_several_assemblies_with_completeness(cli, tmp_path):        # noqa: F811
    k = 21
    e = ks.expected(k)["planted"]
    files, apath, q = write_case(tmp_path, e.case)
    b = named(ks.second_assembly(k)[0], "b")
    (tmp_path / "b.fa").write_bytes(kc.fasta(b))
    (tmp_path / "empty.fa").write_bytes(b"")
    asms = [(apath, q), (str(tmp_path / "b.fa"), b), (str(tmp_path / "empty.fa"), []), (apath, q)]
    for m in (2, 1025):
        w = ks.expect_qv([r for _, r in files], asms, k, m)
        rc, out, err = run(cli, qv_args(k, m, files) + ["--completeness"] + [p for p, _ in asms])
        assert rc == 0 and out == w["stdout"], err[-2000:]
        rows = [ln.split(b"\t") for ln in out.split(b"\n")[1:-1]]
        assert len(set(r[7] for r in rows)) == 1 and rows[0][7:] == rows[3][7:] and rows[2][8] == b"0"        # solid repeats; the clear between two assemblies
        assert (rows[2][9] == b"NA") == (m == 1025)


def test_usage_errors_and_overflow(cli, tmp_path):        # noqa: F811
    k = 21
    f = tmp_path / "t.fa"
    f.write_bytes(b">a\n" + b"ACGT" * 20 + b"\n")
    t, s = str(f), str(tmp_path / "s.tsv")
    fifo = str(tmp_path / "fifo")
    os.mkfifo(fifo)
    bad = [["qv", "--completeness", t, t], ["qv", "--spectra-cn", s, t, t], ["qv", "-r", t, "--spectra-cn", s, t, t], ["qv", "-r", t, "--spectra-cn"],
           ["qv", "--accel=no", "--slots", "100", "-r", t, "--completeness", fifo], ["qv", "--accel=no", "--slots", "100", "-r", t, "--spectra-cn", s, "-"],
           ["qv", "--accel=no", "-r", t, "--completeness", t, fifo]]
    for args in bad:
        rc, out, err = run(cli, args)
        assert rc == 1 and out == b"" and not lines_of(err, b"[qv]") and not os.path.exists(s), args
    rc, out, err = run(cli, ["qv", "--accel=no", "-r", t, "--completeness", fifo])
    assert b"FIFO" in err and b"twice" in err
    rc, out, err = run(cli, ["qv", "--completeness", t, t])
    assert b"go with -r" in err
    rc, out, err = run(cli, ["qv", "-h"])
    assert rc == 0 and b"--completeness" in out and b"--spectra-cn" in out
    # the assembly-only k-mers take slots: a table with room for the reads alone overflows in the copies pass, one ERROR line that names --slots
    e = ks.expected(k)["neighbours_at_load_1"]
    files, apath, q = write_case(tmp_path, e.case)
    for slots, ok in ((e.union, True), (e.union - 1, False), (e.stats[1], False)):
        rc, out, err = run(cli, qv_args(k, 2, files, ["--slots", str(slots), "--completeness"]) + [apath])
        lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
        if ok:
            assert rc == 0 and not lines and out == ks.expect_qv([r for _, r in files], [(apath, q)], k, 2)["stdout"]
        else:
            assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and b"overflowed" in lines[0], (slots, err[-2000:])
    # ... and without the option the same table serves: the reads alone fit
    rc, out, err = run(cli, qv_args(k, 2, files, ["--slots", str(e.stats[1])]) + [apath])
    assert rc == 0 and out == cc.expect_qv([r for _, r in files], [(apath, q)], k, 2)["stdout"]
    # an assembly that holds only read k-mers fits a table of the reads' distinct keys
    (tmp_path / "y.fa").write_bytes(kc.fasta([("y", e.case.reads[0][0])]))
    rc, out, err = run(cli, qv_args(k, 2, files, ["--slots", str(e.stats[1]), "--completeness"]) + [str(tmp_path / "y.fa")])
    cols = out.split(b"\n")[1].split(b"\t")
    assert rc == 0 and cols[7] == cols[8] != b"0" and cols[9] == b"1.000000", err[-2000:]


def test_without_the_options_the_output_is_what_it_was(cli, tmp_path):        # noqa: F811
    """a guard: passes before the feature too"""
    k = 21
    e = ks.expected(k)["seams"]
    files, apath, q = write_case(tmp_path, e.case)
    for m in (1, 2):
        w = cc.expect_qv([r for _, r in files], [(apath, q)], k, m)
        rc, out, err = run(cli, qv_args(k, m, files) + ["-c", str(tmp_path / "c.tsv"), "-b", str(tmp_path / "b.bed"), apath])
        assert rc == 0 and out == w["stdout"] and lines_of(err, b"[qv]") == [w["line"]]
        assert (tmp_path / "c.tsv").read_bytes() == w["contigs"] and (tmp_path / "b.bed").read_bytes() == w["bed"]


def test_the_entry_points_want_their_objects():
    import ctypes as C
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    spec, tot = (C.c_int64 * (ks.CN * ks.BINS))(), (C.c_int64 * 2)()
    assert L.cornetto_kset_copies(None, None, None) == ks.E_ARG and L.cornetto_kset_copies_clear(None, None) == ks.E_ARG
    assert L.cornetto_kset_spectrum(None, None, 0, 1, spec, tot) == ks.E_ARG
    assert cornetto_amd.KSET_CN_BINS == ks.CN


# ---- the kernels' arithmetic on the CPU, under the host sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/kspec_sim.cc: kq_insert_at() + kq_copy_bump() and the cells of csrc/kqv.hpp as kq_copies and kq_spectrum call them; every block
    of exactly its size, under AddressSanitizer and UBSan -> None for an overflow, else ([(spec, {m: (solid, found)}) per assembly], stats, hist,
    solid of the seal with the first m, lost compare-and-swaps)"""
    d = tmp_path_factory.mktemp("kspec_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "kspec_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "kspec_sim")

    def batch(seqs):
        return b"%d\n" % len(seqs) + b"".join(b"%d\n" % len(s) + s + b"\n" for s in seqs)

    def run_sim(k, slots, reads, asms, ms):
        (d / "case.bin").write_bytes(b"%d %d %d\n" % (k, slots, len(reads)) + b"".join(batch(b) for b in reads) + b"%d\n" % len(ms) + b"".join(b"%d\n" % m for m in ms) +
                                     b"%d\n" % len(asms) + b"".join(b"%d\n" % len(a) + b"".join(batch(b) for b in a) for a in asms))
        r = subprocess.run([exe, str(d / "case.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln]
        if ["overflow"] in lines:
            return None
        per, hist = [], [0] * ks.BINS
        for ln in lines:
            if ln[0] == "asm":
                per.append(([[0] * ks.BINS for _ in range(ks.CN)], {}))
            elif ln[0] == "s":
                per[-1][0][int(ln[1])][int(ln[2])] = int(ln[3])
            elif ln[0] == "t":
                per[-1][1][int(ln[1])] = (int(ln[2]), int(ln[3]))
            elif ln[0] == "h":
                hist[int(ln[1])] = int(ln[2])
        sets = [tuple(map(int, ln[1:])) for ln in lines if ln[0] == "set"]
        assert len(sets) == 2 and sets[0] == sets[1]
        return per, sets[0], hist, int(next(ln for ln in lines if ln[0] == "solid")[1]), int(next(ln for ln in lines if ln[0] == "lost")[1])
    return run_sim


@pytest.mark.parametrize("k", ks.KS)
def test_sim_cases(sim, k):
    exp = ks.expected(k)
    for name, e in exp.items():
        got = sim(k, ks.slots_of(e), e.case.reads, [e.case.asm], e.case.ms)
        assert got[:4] == ([(e.spec, e.totals)], e.stats, e.hist, e.totals[e.case.ms[0]][0]), name
        assert got[4] > 0 or name.startswith("one_key")          # compare-and-swaps were lost and retried
    # a table with one slot too few is a status; the reads' distinct keys are enough for an assembly that holds only read k-mers
    e = exp["neighbours_at_load_1"]
    assert sim(k, e.union - 1, e.case.reads, [e.case.asm], (1,)) is None and sim(k, e.stats[1], e.case.reads, [e.case.asm], (1,)) is None
    assert sim(k, e.stats[1], e.case.reads, [[e.case.reads[0][:1]]], (1,)) is not None
    # two assemblies: the second equals that of a set that saw only B, although A's assembly-only keys are still in the table
    p, B = exp["planted"], ks.second_assembly(k)
    R, _ = ks.counter(p.case.reads, k)
    Bc, _ = ks.counter(B, k)
    both = sim(k, ks.slots_of(p) + 1000, p.case.reads, [p.case.asm, B, p.case.asm], (2,))
    alone = sim(k, ks.slots_of(p) + 1000, p.case.reads, [B], (2,))
    assert both[0][1] == alone[0][0] == (ks.spectrum(R, Bc), {2: ks.totals(R, Bc, 2)}) and both[0][0] == both[0][2] == (p.spec, {2: p.totals[2]})
    assert both[0][1][0][0][0] == 0 and both[1:4] == alone[1:4]
