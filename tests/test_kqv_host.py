"""CPU: `cornetto qv` on the host path (--accel=no / CORNETTO_ACCEL=no) with the product binary and the sanitized build of the same host C,
byte for byte against the formatter of tests/kqv_cases.py — stdout, -c, -b, the stderr truth line, the usage errors, the overflow error — and
the arithmetic of the kernels (csrc/kqv.hpp) as a CPU program under the host sanitizers.  The device path is tests/test_gpu_kqv.py's.
Every test here fails on the parent commit: it has no qv, no kqv.hpp and none of the symbols."""
import gzip
import os
import subprocess

import pytest

import cornetto_amd
import kqv_cases as kc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def named(seqs, tag="c"):
    return [("%s%d" % (tag, i), s) for i, s in enumerate(seqs)]


def write_case(d, truth, query):
    """-> (truth paths, assembly path, truth records per file, assembly records)"""
    tfiles = [named(b, "t%d_" % i) for i, b in enumerate(truth)]
    paths = []
    for i, recs in enumerate(tfiles):
        p = d / ("truth%d.fa" % i)
        p.write_bytes(kc.fasta(recs, width=(0, 60, 7)[i % 3]))
        paths.append(str(p))
    q = named(query)
    a = d / "asm.fa"
    a.write_bytes(kc.fasta(q, width=70))
    return paths, str(a), tfiles, q


def qv_args(k, tpaths, extra=()):
    args = ["qv", "--accel=no", "-k", str(k)]
    for p in tpaths[1:]:
        args += ["-t", p]
    return args + list(extra) + [tpaths[0]]


def truth_lines(err):
    return [ln for ln in err.split(b"\n") if ln.startswith(b"[qv]")]


def test_the_restatement_agrees_with_the_words_of_the_rule():
    import random
    rng = random.Random(5)
    for k in kc.KS:
        for n in (0, k - 1, k, 300):
            s = bytearray(kc.dna(rng, n))
            for o in rng.sample(range(n), min(n, 4)):
                s[o] = rng.choice(b"Nn-acgtX")
            assert kc.kmers_of(bytes(s), k) == kc.slow_kmers_of(bytes(s), k)
        # a single substitution away from the ends: exactly k missing positions and one row of width 2k - 1; at the ends it is clipped
        cs = dict((n, (t, q)) for n, t, q in kc.cases(k))
        t, q = cs["one_substitution"]
        S, _ = kc.truth_set(t[0], k)
        kmers, missing, rows = kc.query(S, q, k)
        L = len(t[0][0])
        assert missing[:4] == [k, k, 1, 1] and missing[4] == 2 and kmers == [L - k + 1] * len(q)
        assert rows[:4] == [(0, kc.TILE - k, kc.TILE + k - 1), (1, kc.TILE - k + 1, kc.TILE + k), (2, 0, k), (3, L - k, L)]
        # two substitutions k - 1 and k apart are one run of missing positions, k + 1 apart two runs whose spans overlap: one row each; 2k - 1
        # apart the two spans are book-ended and still one row, 2k apart there is a base between them: two rows
        t, q = cs["two_substitutions"]
        _, _, rows = kc.query(kc.truth_set(t[0], k)[0], q, k)
        assert [sum(1 for r in rows if r[0] == c) for c in range(18)] == [1, 1, 1, 1, 2, 2] * 3
        assert kc.query(kc.truth_set(cs["reverse_complement"][0][0], k)[0], cs["reverse_complement"][1], k)[1] == [0, 0, 0]
        assert len(kc.truth_set(cs["homopolymer"][0][0], k)[0]) == 1
    assert kc.qv_strings(0, 0, 21) == ("NA", "NA") and kc.qv_strings(10, 0, 21) == ("0", "inf") and kc.qv_strings(1000000, 21, 21) == ("1.000e-06", "60.00")


@pytest.mark.parametrize("k", kc.KS)
def test_host_path_cases(cli, tmp_path, k):        # noqa: F811
    for name, truth, query in kc.cases(k):
        d = tmp_path / name
        d.mkdir()
        tpaths, apath, tfiles, q = write_case(d, truth, query)
        w = kc.expect_cli(tfiles, [(apath, q)], k)
        rc, out, err = run(cli, qv_args(k, tpaths, ["-c", str(d / "c.tsv"), "-b", str(d / "b.bed")]) + [apath])
        assert rc == 0 and out == w["stdout"], (name, err[-2000:])
        assert (d / "c.tsv").read_bytes() == w["contigs"] and (d / "b.bed").read_bytes() == w["bed"], name
        assert truth_lines(err) == [w["truth_line"]], name


def test_default_k_several_assemblies_and_the_environment_switch(cli, tmp_path):        # noqa: F811
    cs = dict((n, (t, q)) for n, t, q in kc.cases(21))
    tpaths, apath, tfiles, q = write_case(tmp_path, *cs["one_substitution"])
    b = tmp_path / "second.fa.gz"
    q2 = named(cs["two_substitutions"][1], "z")
    b.write_bytes(gzip.compress(kc.fasta(q2, width=80)))
    e = tmp_path / "empty.fa"
    e.write_bytes(b"")
    files = [(apath, q), (str(b), q2), (str(e), []), (apath, q)]
    w = kc.expect_cli(tfiles, files, 21)
    env = dict(os.environ, CORNETTO_ACCEL="no")
    p = subprocess.run([cli, "qv", tpaths[0]] + [f for f, _ in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and p.stdout == w["stdout"] and truth_lines(p.stderr) == [w["truth_line"]]
    assert b"\tNA\tNA\n" in p.stdout and p.stderr.count(b"\n[main] ") >= 2          # an assembly without k-mers; the usual footer follows
    # a gzip truth is sized by a pass over its records
    g = tmp_path / "truth.fa.gz"
    g.write_bytes(gzip.compress(kc.fasta(tfiles[0])))
    rc, out, err = run(cli, ["qv", "--accel=no", str(g), apath])
    assert rc == 0 and out == kc.expect_cli(tfiles, [(apath, q)], 21)["stdout"]


def test_table_sizes_and_overflow(cli, tmp_path):        # noqa: F811
    k = 21
    cs = dict((n, (t, q)) for n, t, q in kc.cases(k))
    truth, query = cs["two_batches"]
    tpaths, apath, tfiles, q = write_case(tmp_path, truth, query)
    w = kc.expect_cli(tfiles, [(apath, q)], k)
    for slots in (w["distinct"], w["distinct"] + 1, 10 * w["distinct"]):          # load 1.0: chains that wrap; the results are exact
        rc, out, err = run(cli, qv_args(k, tpaths, ["--slots", str(slots), "-b", str(tmp_path / "b.bed")]) + [apath])
        assert rc == 0 and out == w["stdout"] and (tmp_path / "b.bed").read_bytes() == w["bed"] and truth_lines(err) == [w["truth_line"]], slots
    for slots in (w["distinct"] - 1, 1):
        rc, out, err = run(cli, qv_args(k, tpaths, ["--slots", str(slots)]) + [apath])
        lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
        assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and not truth_lines(err), (slots, err)
    hp, hq = cs["homopolymer"]
    tpaths, apath, tfiles, q = write_case(tmp_path, hp, hq)
    rc, out, err = run(cli, qv_args(k, tpaths, ["--slots", "1"]) + [apath])
    assert rc == 0 and out == kc.expect_cli(tfiles, [(apath, q)], k)["stdout"] and b"1 distinct" in truth_lines(err)[0]


def test_usage_errors_and_help(cli, tmp_path):        # noqa: F811
    f = tmp_path / "t.fa"
    f.write_bytes(b">a\n" + b"ACGT" * 20 + b"\n")
    t = str(f)
    bad = [["qv"], ["qv", t], ["qv", "-k", "20", t, t], ["qv", "-k", "9", t, t], ["qv", "-k", "33", t, t], ["qv", "-k", "x", t, t], ["qv", "--slots", "0", t, t],
           ["qv", "--slots", "1x", t, t], ["qv", "-c", str(tmp_path / "c"), t, t, t], ["qv", "-b", str(tmp_path / "b"), t, t, t], ["qv", "--accel=maybe", t, t],
           ["qv", "--accel=no", "-", t], ["qv", "--accel=no", "-t", "-", t, t], ["qv", "--nonsense", t, t]]
    for args in bad:
        rc, out, err = run(cli, args)
        assert rc == 1 and out == b"" and not truth_lines(err), args
    os.mkfifo(str(tmp_path / "fifo"))
    rc, out, err = run(cli, ["qv", "--accel=no", str(tmp_path / "fifo"), t])
    assert rc == 1 and out == b"" and b"--slots" in err
    rc, out, err = run(cli, ["qv", "--accel=no", str(tmp_path / "missing.fa"), t])
    assert rc == 1 and out == b""
    rc, out, err = run(cli, ["qv", "-h"])
    assert rc == 0 and out.startswith(b"Usage: cornetto qv") and b"--slots" in out
    rc, out, err = run(cli, ["--help"])
    assert [ln for ln in out.split(b"\n") if ln.strip().startswith(b"qv ")] and out.index(b"eval:") < out.index(b" qv ") < out.index(b"misc:")


def test_the_entry_points_want_their_objects():
    import ctypes as C
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    p = C.c_void_p()
    assert L.cornetto_kset_open(None, 21, 100, C.byref(p)) == -3 and L.cornetto_kset_add(None, None, None) == -3
    assert L.cornetto_kset_query(None, None, None, None, None, None, None) == -3
    st = (C.c_int64 * 3)(7, 7, 7)
    L.cornetto_kset_stats(None, st)
    L.cornetto_kset_free(None, None)
    assert list(st) == [7, 7, 7] and cornetto_amd.KQV_TILE == kc.TILE


# ---- the kernels' arithmetic on the CPU, under the host sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/kqv_sim.cc: kq_run, kq_insert, kq_lookup, kq_bit and the run words of csrc/kqv.hpp as the kernels call them; every contig, the
    table, the bitmap and the rows in a heap block of exactly its size, under AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("kqv_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "kqv_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "kqv_sim")

    def batch(seqs):
        return b"%d\n" % len(seqs) + b"".join(b"%d\n" % len(s) + s + b"\n" for s in seqs)

    def run_sim(k, slots, truth, query):
        (d / "case.bin").write_bytes(b"%d %d %d\n" % (k, slots, len(truth)) + b"".join(batch(b) for b in truth) + batch(query))
        r = subprocess.run([exe, str(d / "case.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        lines = r.stdout.decode().split("\n")
        if lines[0] == "overflow":
            return None
        cs = [tuple(map(int, ln.split()[1:])) for ln in lines if ln.startswith("c ")]
        rows = [tuple(map(int, ln.split()[1:])) for ln in lines if ln.startswith("r ")]
        return tuple(map(int, lines[0].split()[1:])), [c[0] for c in cs], [c[1] for c in cs], rows
    return run_sim


def expect_sim(k, truth, query):
    S, n_pos = kc.truth_set([s for b in truth for s in b], k)
    return ((n_pos, len(S)),) + kc.query(S, query, k)


@pytest.mark.parametrize("k", kc.KS)
def test_sim_cases(sim, k):
    for name, truth, query in kc.cases(k):
        exp = expect_sim(k, truth, query)
        distinct = exp[0][1]
        assert sim(k, 2 * exp[0][0] + 1, truth, query) == exp, name
        if name in ("two_batches", "tile_lengths", "homopolymer", "tandem_repeat", "short_contigs"):
            assert sim(k, distinct, truth, query) == exp, name                      # load 1.0
            if distinct > 1:
                assert sim(k, distinct - 1, truth, query) is None, name             # a table that is too small is a status
                assert sim(k, 1, truth, query) is None, name


def test_sim_moderate(sim):
    truth, q = kc.moderate(21)
    assert sim(21, 500009, [truth[:3], truth[3:]], q) == expect_sim(21, [truth], q)
