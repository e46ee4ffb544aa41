"""CPU: `cornetto trioeval` on the host path (--accel=no / CORNETTO_ACCEL=no) with the product binary and the sanitized build of the same host C,
byte for byte against the formatter of tests/ktrio_cases.py — stdout, -c, the stderr parents line, the usage errors, the overflow error — and the
tagged table and the ordered pass of the kernels (csrc/kqv.hpp, csrc/ktrio.hpp) as a CPU program under the host sanitizers.  The device path is
tests/test_gpu_ktrio.py's.  The CLI and sim tests fail on the parent commit: it has no trioeval, no ktrio.hpp and none of the symbols."""
import gzip
import os
import subprocess

import pytest

import bgcomp_cases as bg
import cornetto_amd
import kqv_cases as kc
import ktrio_cases as tc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"#file\tcontigs\tbases\tkmers\tpat\tmat\tpairs\tswitches\tswitch_rate\thamming\thamming_rate\n"


def named(seqs, tag="c"):
    return [("%s%d" % (tag, i), s) for i, s in enumerate(seqs)]


def pack(kind, text):
    return {"plain": text, "gzip": gzip.compress(text), "bgzf": bg.bgzf(text, bg.seeded_sizes(len(text), 5, 1, 3000))}[kind]


def write_case(d, batches, query, kinds=("plain",)):
    """a file per parental batch, in the form kinds[i % len(kinds)] -> (pat paths, mat paths, assembly path, pat records per file, mat records per
    file, assembly records)"""
    paths, files = {tc.PAT: [], tc.MAT: []}, {tc.PAT: [], tc.MAT: []}
    for i, (tag, seqs) in enumerate(batches):
        recs = named(seqs, "p%d_" % i)
        kind = kinds[i % len(kinds)]
        p = d / ("parent%d.fa%s" % (i, "" if kind == "plain" else ".gz"))
        p.write_bytes(pack(kind, kc.fasta(recs, width=(0, 60, 7)[i % 3])))
        paths[tag].append(str(p))
        files[tag].append(recs)
    for tag in (tc.PAT, tc.MAT):          # the two positional arguments are always there
        if not paths[tag]:
            p = d / ("none%d.fa" % tag)
            p.write_bytes(b"")
            paths[tag].append(str(p))
            files[tag].append([])
    q = named(query)
    kind = kinds[len(batches) % len(kinds)]
    a = d / ("asm.fa" + ("" if kind == "plain" else ".gz"))
    a.write_bytes(pack(kind, kc.fasta(q, width=70)))
    return paths[tc.PAT], paths[tc.MAT], str(a), files[tc.PAT], files[tc.MAT], q


def trio_args(k, ppaths, mpaths, extra=()):
    args = ["trioeval", "--accel=no", "-k", str(k)]
    for p in ppaths[1:]:
        args += ["-P", p]
    for p in mpaths[1:]:
        args += ["-M", p]
    return args + list(extra) + [ppaths[0], mpaths[0]]


def parent_lines(err):
    return [ln for ln in err.split(b"\n") if ln.startswith(b"[trioeval]")]


def test_the_restatement_and_the_cases_say_what_they_claim():
    for k in tc.KS:
        e = tc.expected(k)
        for name, (batches, query, st, rows) in e.items():
            for r in rows:          # the identity of the rule: every marker but a contig's first has exactly one pair
                assert sum(r[3:]) == max(r[1] + r[2] - 1, 0) and r[1] + r[2] <= r[0], name
        # markers at 63 | 64 and at TILE - 1 | TILE: the four type combinations are the four pairs, one each
        for name in ("word_seam", "tile_seam"):
            rows = e[name][3]
            assert [r[1:] for r in rows[:4]] == [[2, 0, 1, 0, 0, 0], [1, 1, 0, 1, 0, 0], [1, 1, 0, 0, 1, 0], [0, 2, 0, 0, 0, 1]], name
            assert rows[4][1:] == [2, 2, 0, 1, 1, 1] and rows[5][1:] == [1, 1, 0, 0, 1, 0] and rows[6][1:] == [0, 1, 0, 0, 0, 0], name
        rows = e["last_position_and_short_contigs"][3]
        assert [r[:3] for r in rows] == [[tc.TILE + 6, 0, 1], [tc.TILE, 1, 0], [tc.TILE + 1, 1, 0], [1, 0, 1], [0, 0, 0], [0, 0, 0], [1, 0, 0]]
        assert all(sum(r[3:]) == 0 for r in rows)
        rows = e["no_pair_across_contigs"][3]
        assert [r[1:] for r in rows] == [[2, 0, 1, 0, 0, 0], [0] * 6, [1, 1, 0, 0, 1, 0], [0, 1, 0, 0, 0, 0], [0] * 6, [1, 0, 0, 0, 0, 0]]
        rows = e["long_marker_free_stretches"][3]
        assert [r[1:] for r in rows] == [[1, 1, 0, 1, 0, 0], [0, 1, 0, 0, 0, 0], [1, 2, 0, 0, 1, 1], [2, 0, 1, 0, 0, 0]]
        b, q, st, rows = e["both_neither_and_reverse_complement"]
        assert rows[0][1:] == [2, 2, 1, 1, 0, 1] and rows[1][1:] == [2, 2, 1, 0, 1, 1] and rows[2] == rows[0]      # pat 50, (both 100), pat 200, mat 300, mat 320
        assert e["invalid_between_markers"][3][0][1:] == [2, 2, 0, 1, 1, 1] and e["invalid_between_markers"][3][1][1:] == [2, 2, 0, 1, 1, 1]
        rows = e["homopolymer"][3]
        assert rows[0] == [2 * tc.TILE + 101 - k, 2 * tc.TILE + 101 - k, 0, 2 * tc.TILE + 100 - k, 0, 0, 0] and rows[2][4] == 1 and rows[2][5] == 0
        assert e["homopolymer"][2][1] == 2
        assert sum(r[4] + r[5] for r in e["mosaic"][3]) >= 5 and sum(r[4] + r[5] for r in e["dense_random"][3]) > 500
    assert tc.rate(0, 0) == "NA" and tc.rate(1, 3) == "0.333333" and tc.rate(0, 5) == "0.000000"


@pytest.mark.parametrize("k", tc.KS)
def test_host_path_cases(cli, tmp_path, k):        # noqa: F811
    for i, (name, batches, query) in enumerate(tc.cases(k)):
        d = tmp_path / name
        d.mkdir()
        kinds = (("plain",), ("plain", "gzip", "bgzf"), ("bgzf", "plain"), ("gzip",))[i % 4]
        pp, mp, apath, pf, mf, q = write_case(d, batches, query, kinds)
        w = tc.expect_cli(pf, mf, [(apath, q)], k, known=tc.expected(k)[name][2:])
        rc, out, err = run(cli, trio_args(k, pp, mp, ["-c", str(d / "c.tsv")]) + [apath])
        assert rc == 0 and out == w["stdout"], (name, err[-2000:])
        assert (d / "c.tsv").read_bytes() == w["contigs"], name
        assert parent_lines(err) == [w["parents_line"]], name


def test_default_k_several_assemblies_and_the_environment_switch(cli, tmp_path):        # noqa: F811
    cs = dict((n, (b, q)) for n, b, q in tc.cases(21))
    pp, mp, apath, pf, mf, q = write_case(tmp_path, *cs["mosaic"], kinds=("plain", "bgzf", "gzip"))
    assert len(pp) > 1 and len(mp) > 1          # several -P and -M files
    b = tmp_path / "second.fa.gz"
    q2 = named(cs["dense_random"][1], "z")
    b.write_bytes(gzip.compress(kc.fasta(q2, width=80)))
    e = tmp_path / "empty.fa"
    e.write_bytes(b"")
    files = [(apath, q), (str(b), q2), (str(e), []), (apath, q)]
    w = tc.expect_cli(pf, mf, files, 21)
    env = dict(os.environ, CORNETTO_ACCEL="no")
    args = [a for a in trio_args(21, pp, mp) if a not in ("--accel=no", "-k", "21")]
    p = subprocess.run([cli] + args + [f for f, _ in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and p.stdout == w["stdout"] and parent_lines(p.stderr) == [w["parents_line"]]
    assert b"\tNA\t0\tNA\n" in p.stdout and p.stdout.startswith(HEADER)          # an assembly without markers: both rates NA


def test_table_sizes_and_overflow(cli, tmp_path):        # noqa: F811
    k = 21
    cs = dict((n, (b, q)) for n, b, q in tc.cases(k))
    pp, mp, apath, pf, mf, q = write_case(tmp_path, *cs["tags_arrive_in_either_order"])
    w = tc.expect_cli(pf, mf, [(apath, q)], k)
    for slots in (w["distinct"], w["distinct"] + 1, 10 * w["distinct"]):          # load 1.0: chains that wrap; the results are exact
        rc, out, err = run(cli, trio_args(k, pp, mp, ["--slots", str(slots), "-c", str(tmp_path / "c.tsv")]) + [apath])
        assert rc == 0 and out == w["stdout"] and (tmp_path / "c.tsv").read_bytes() == w["contigs"] and parent_lines(err) == [w["parents_line"]], slots
    for slots in (w["distinct"] - 1, 1):
        rc, out, err = run(cli, trio_args(k, pp, mp, ["--slots", str(slots)]) + [apath])
        lines = [ln for ln in err.split(b"\n") if b"ERROR" in ln]
        assert rc == 1 and out == b"" and len(lines) == 1 and b"--slots" in lines[0] and not parent_lines(err), (slots, err)


def test_usage_errors_and_help(cli, tmp_path):        # noqa: F811
    f = tmp_path / "t.fa"
    f.write_bytes(b">a\n" + b"ACGT" * 20 + b"\n")
    t = str(f)
    c = str(tmp_path / "c")
    bad = [["trioeval"], ["trioeval", t], ["trioeval", t, t], ["trioeval", "-k", "20", t, t, t], ["trioeval", "-k", "9", t, t, t], ["trioeval", "-k", "33", t, t, t],
           ["trioeval", "-k", "x", t, t, t], ["trioeval", "--slots", "0", t, t, t], ["trioeval", "--slots", "1x", t, t, t], ["trioeval", "-c", c, t, t, t, t],
           ["trioeval", "--accel=maybe", t, t, t], ["trioeval", "--accel=no", "-", t, t], ["trioeval", "--accel=no", "-M", "-", t, t, t], ["trioeval", "--nonsense", t, t, t]]
    for args in bad:
        rc, out, err = run(cli, args)
        assert rc == 1 and out == b"" and not parent_lines(err), args
    os.mkfifo(str(tmp_path / "fifo"))
    rc, out, err = run(cli, ["trioeval", "--accel=no", t, str(tmp_path / "fifo"), t])
    assert rc == 1 and out == b"" and b"--slots" in err
    rc, out, err = run(cli, ["trioeval", "--accel=no", t, str(tmp_path / "missing.fa"), t])          # a missing mat file
    assert rc == 1 and out == b""
    rc, out, err = run(cli, ["trioeval", "--accel=no", "--slots", "1000", t, str(tmp_path / "missing.fa"), t])
    assert rc == 1 and out == b""
    rc, out, err = run(cli, ["trioeval", "-h"])
    assert rc == 0 and out.startswith(b"Usage: cornetto trioeval") and b"--slots" in out and b"-M FILE" in out
    rc, out, err = run(cli, ["--help"])
    assert [ln for ln in out.split(b"\n") if ln.strip().startswith(b"trioeval ")] and out.index(b"eval:") < out.index(b" trioeval ") < out.index(b"misc:")


def test_the_entry_points_want_their_objects():
    import ctypes as C
    if not os.path.exists(cornetto_amd.LIB_PATH):
        cornetto_amd.build()
    L = cornetto_amd.lib()
    assert L.cornetto_kset_add_tag(None, None, None, 1) == tc.E_ARG and L.cornetto_kset_phase(None, None, None, None) == tc.E_ARG
    assert hasattr(cornetto_amd.Kset, "phase") and C.sizeof(C.c_int64) * 7 == 56


# ---- the kernels' arithmetic on the CPU, under the host sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/ktrio_sim.cc: kq_run, kq_insert_tag, kq_lookup_tag and kq_bit of csrc/kqv.hpp and the word, wave and seam logic of csrc/ktrio.hpp
    as the kernels call them; every contig, the table, the bitmaps, the tile bytes and the counters in a heap block of exactly its size, under
    AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("ktrio_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "ktrio_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "ktrio_sim")

    def batch(tag, seqs):
        return b"%d %d\n" % (tag, len(seqs)) + b"".join(b"%d\n" % len(s) + s + b"\n" for s in seqs)

    def run_sim(k, slots, batches, query):
        (d / "case.bin").write_bytes(b"%d %d %d\n" % (k, slots, len(batches)) + b"".join(batch(t, b) for t, b in batches) + batch(0, query))
        r = subprocess.run([exe, str(d / "case.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        lines = r.stdout.decode().split("\n")
        if lines[0] == "overflow":
            return None
        return tuple(map(int, lines[0].split()[1:])), [list(map(int, ln.split()[1:])) for ln in lines if ln.startswith("c ")]
    return run_sim


@pytest.mark.parametrize("k", tc.KS)
def test_sim_cases(sim, k):
    for name, (batches, query, st, rows) in tc.expected(k).items():
        assert sim(k, 2 * st[0] + 1, batches, query) == (st, rows), name
        assert sim(k, 2 * st[0] + 1, batches[::-1], query) == (st, rows), name          # the parents in the other order
        if name in tc.FULL_TABLE_CASES:
            assert sim(k, st[1], batches, query) == (st, rows), name                    # load 1.0
            if st[1] > 1:
                assert sim(k, st[1] - 1, batches, query) is None, name                  # a table that is too small is a status
