"""GPU: the tagged k-mer set and the ordered pass of `cornetto trioeval` (csrc/ktrio.hip) against the plain-Python sets of tests/ktrio_cases.py:
exact equality of the 7 counts per contig and of the set's statistics through the binding, and of the bytes through the CLI on the device and
with --accel=no.  The cases are the smallest shapes at which the kernels can go wrong (word and tile seams, marker-free stretches of more than
a round of the seam walk, contig ends, tags that arrive in either order, tables at load 1.0 and one slot too few), each for k = 11, 21 and 31;
the expected values are computed once per k and shared."""
import gzip
import subprocess

import pytest

import cornetto_amd
import kqv_cases as kc
import ktrio_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def build(acc, k, slots, batches):
    s = acc.kset(k, slots)
    for tag, b in batches:
        a = acc.asm_upload(b)
        try:
            s.add(a, tag=tag)
        finally:
            a.close()
    return s


def phase(acc, s, query):
    a = acc.asm_upload(query)
    r = s.phase(a)
    a.close()
    assert r.shape == (len(query), 7) and str(r.dtype) == "int64"
    return [list(map(int, row)) for row in r]


def halves(batches):
    """every batch split into two of the same tag"""
    out = []
    for tag, b in batches:
        out += [(tag, b[:len(b) // 2]), (tag, b[len(b) // 2:])]
    return out


@pytest.mark.parametrize("k", tc.KS)
def test_cases(acc, k):
    for name, (batches, query, st, rows) in tc.expected(k).items():
        slots = 2 * st[0] + 1
        s = build(acc, k, slots, batches)
        assert s.stats == st + (slots,), name          # positions and distinct of the union
        assert phase(acc, s, query) == rows, name
        s.close()
    names = [n for n, _ in acc.last_timing()]
    assert {"kt_mark", "kt_tile", "kt_seam"} <= set(names) and "kq_query" not in names and "kt_insert" not in names


@pytest.mark.parametrize("k", tc.KS)
def test_order_batches_full_tables_and_overflow(acc, k):
    e = tc.expected(k)
    for name in tc.FULL_TABLE_CASES:
        batches, query, st, rows = e[name]
        for b in (batches[::-1], halves(batches)):               # the parents in the other order, and in split batches
            s = build(acc, k, 2 * st[0] + 1, b)
            assert s.stats[:2] == st and phase(acc, s, query) == rows, name
            s.close()
        s = build(acc, k, st[1], batches)                        # load 1.0: chains that wrap, absent keys walk the whole table
        assert s.stats == st + (st[1],) and phase(acc, s, query) == rows, name
        s.close()
        if st[1] > 1:                                            # one slot too few: a status, never a hang
            with pytest.raises(cornetto_amd.AccelError) as ei:
                build(acc, k, st[1] - 1, batches)
            assert ei.value.status == tc.E_NOMEM, name
    batches, query, st, rows = e["word_seam"]                    # the handle stays usable after the overflow
    s = build(acc, k, 2 * st[0] + 1, batches)
    assert phase(acc, s, query) == rows
    s.close()


def test_arguments_empty_inputs_and_mixing(acc):
    k = 21
    batches, query, st, rows = tc.expected(k)["mosaic"]
    s = build(acc, k, 2 * st[0] + 1, batches)
    assert phase(acc, s, []) == [] and phase(acc, s, [b"", b"ACGT", b"A" * (k - 1)]) == [[0] * 7] * 3          # 0 contigs, 0 tiles, shorter than k
    for _ in range(2):                                           # the same set, assemblies in turn
        assert phase(acc, s, query) == rows and phase(acc, s, query[1:2]) == rows[1:2]
    a = acc.asm_upload(query[:1])
    for bad in (3, -1, 4):
        with pytest.raises(cornetto_amd.AccelError) as ei:
            s.add(a, tag=bad)
        assert ei.value.status == tc.E_ARG
    for call in (lambda: s.add(a), lambda: s.query(a)):          # a tagged set refuses the plain calls
        with pytest.raises(cornetto_amd.AccelError) as ei:
            call()
        assert ei.value.status == tc.E_UNSUPPORTED and "tagged" in str(ei.value)
    assert phase(acc, s, query) == rows
    s.close()
    p = acc.kset(k, 100000)
    p.add(a)
    for call in (lambda: p.add(a, tag=1), lambda: p.phase(a)):   # a plain set refuses the tagged calls
        with pytest.raises(cornetto_amd.AccelError) as ei:
            call()
        assert ei.value.status == tc.E_UNSUPPORTED and "plain" in str(ei.value)
    assert int(p.query(a)[0][0]) == rows[0][0]                   # and stays usable as what it is
    p.close()
    a.close()


def test_nothing_depends_on_what_the_memory_held(dacc):
    """the table over memory that held 0x00 and then 0x5a, and the handle's workspaces — counters, bitmaps, tile bytes — filled with both
    between two calls"""
    import torch
    import selftest_bind as st
    k = 21
    batches, query, stt, rows = tc.expected(k)["mosaic"]
    slots = 2 * stt[0] + 1
    for byte in (0x00, 0x5A):
        junk = torch.full((slots * 8,), byte, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        del junk
        torch.cuda.empty_cache()
        s = build(dacc, k, slots, batches)
        assert s.stats == stt + (slots,) and phase(dacc, s, query) == rows, byte
        filled, _, _ = st.ws_fill(dacc, byte)
        assert {"WS_KT_CNT", "WS_KT_MAP"} <= set(filled)
        assert phase(dacc, s, query) == rows, byte
        st.ws_fill(dacc, 0xFF)
        assert phase(dacc, s, query[:1]) == rows[:1], byte
        assert phase(dacc, s, query) == rows, byte
        s.close()


@pytest.mark.parametrize("k", tc.KS)
def test_cli_device_and_host_print_the_same_bytes(tmp_path, k):
    """every case of k but the longest in one pat.fa, a gzip -P file, one mat.fa, a gzip -M file and one assembly: the device's bytes, the host
    path's and the formatter's; then the longest case by itself"""
    e = dict(tc.expected(k))
    batches, query, st, rows = e.pop("long_marker_free_stretches")
    files = {}
    for tag, t in ((tc.PAT, "p"), (tc.MAT, "m")):
        first = [s for n in sorted(e) for g, b in e[n][0][:2] if g == tag for s in b]
        rest = [s for n in sorted(e) for g, b in e[n][0][2:] if g == tag for s in b]
        files[t] = [[("%s%d" % (t, i), s) for i, s in enumerate(first)], [("%sx%d" % (t, i), s) for i, s in enumerate(rest)]]
        (tmp_path / (t + "0.fa")).write_bytes(kc.fasta(files[t][0], width=60))
        (tmp_path / (t + "1.fa.gz")).write_bytes(gzip.compress(kc.fasta(files[t][1])))
    q = [("q%d" % i, s) for i, s in enumerate(s for n in sorted(e) for s in e[n][1])]
    (tmp_path / "q.fa").write_bytes(kc.fasta(q, width=80))
    apath = str(tmp_path / "q.fa")
    w = tc.expect_cli(files["p"], files["m"], [(apath, q)], k)
    pos = [str(tmp_path / "p0.fa"), str(tmp_path / "m0.fa")]
    for mode in ("dev", "host"):
        args = [cornetto_amd.CLI_PATH, "trioeval", "-k", str(k), "-P", str(tmp_path / "p1.fa.gz"), "-M", str(tmp_path / "m1.fa.gz"), "-c", str(tmp_path / (mode + ".tsv"))]
        p = subprocess.run(args + (["--accel=no"] if mode == "host" else []) + pos + [apath], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and p.stdout == w["stdout"], (mode, p.stderr[-2000:])
        assert (tmp_path / (mode + ".tsv")).read_bytes() == w["contigs"], mode
        assert [ln for ln in p.stderr.split(b"\n") if ln.startswith(b"[trioeval]")] == [w["parents_line"]], mode
    lp, lm = ([[("%s%d" % (t, i), s) for i, s in enumerate(s for g, b in batches if g == tag for s in b)]] for tag, t in ((tc.PAT, "lp"), (tc.MAT, "lm")))
    lq = [("lq%d" % i, s) for i, s in enumerate(query)]
    for name, recs in (("lp.fa", lp[0]), ("lm.fa", lm[0]), ("lq.fa", lq)):
        (tmp_path / name).write_bytes(kc.fasta(recs, width=100))
    w = tc.expect_cli(lp, lm, [(str(tmp_path / "lq.fa"), lq)], k, known=(st, rows))
    p = subprocess.run([cornetto_amd.CLI_PATH, "trioeval", "-k", str(k), "-c", str(tmp_path / "l.tsv")] + [str(tmp_path / n) for n in ("lp.fa", "lm.fa", "lq.fa")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout == w["stdout"] and (tmp_path / "l.tsv").read_bytes() == w["contigs"], p.stderr[-2000:]
    if k == 21:      # two assemblies in argument order; a table one slot too small: one ERROR line that names --slots, nothing on stdout
        q2 = [("r%d" % i, s) for i, s in enumerate(e["mosaic"][1])]
        (tmp_path / "q2.fa").write_bytes(kc.fasta(q2, width=61))
        apath = str(tmp_path / "q2.fa")
        w2 = tc.expect_cli(files["p"][:1], files["m"][:1], [(apath, q2), (pos[0], files["p"][0])], k)
        p = subprocess.run([cornetto_amd.CLI_PATH, "trioeval"] + pos + [apath, pos[0]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and p.stdout == w2["stdout"], p.stderr[-2000:]
        p = subprocess.run([cornetto_amd.CLI_PATH, "trioeval", "--slots", str(w2["distinct"] - 1)] + pos + [apath], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        lines = [ln for ln in p.stderr.split(b"\n") if b"ERROR" in ln]
        assert p.returncode == 1 and p.stdout == b"" and len(lines) == 1 and b"--slots" in lines[0], p.stderr[-2000:]
