"""GPU: the k-mer set of `cornetto qv` (csrc/kqv.hip) against the plain-Python set of tests/kqv_cases.py: exact equality of kmers, missing,
distinct and the rows through the binding, and of the bytes through the CLI on the device and with --accel=no.  The cases are the smallest
shapes at which the kernels can go wrong (contig ends, tile and run seams, invalid bytes, tables at load 1.0 and beyond), each for k = 11, 21
and 31; the expected values are computed once per k and shared."""
import functools
import gzip
import subprocess

import numpy as np
import pytest

import cornetto_amd
import kqv_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def expected(k):
    """{name: (truth, query, (positions, distinct), kmers, missing, rows)}"""
    out = {}
    for name, truth, query in kc.cases(k):
        S, n_pos = kc.truth_set([s for b in truth for s in b], k)
        out[name] = (truth, query, (n_pos, len(S))) + kc.query(S, query, k)
    return out


def build(acc, k, slots, truth):
    s = acc.kset(k, slots)
    for b in truth:
        a = acc.asm_upload(b)
        s.add(a)
        a.close()
    return s


def probe(acc, s, query, runs=True):
    a = acc.asm_upload(query)
    r = s.query(a, runs=runs)
    a.close()
    if not runs:
        return list(map(int, r[0])), list(map(int, r[1]))
    return list(map(int, r[0])), list(map(int, r[1])), [tuple(map(int, x)) for x in r[2]]


@pytest.mark.parametrize("k", kc.KS)
def test_cases(acc, k):
    for name, (truth, query, st, kmers, missing, rows) in expected(k).items():
        s = build(acc, k, 2 * st[0] + 1, truth)
        assert s.stats == st + (2 * st[0] + 1,), name
        assert probe(acc, s, query) == (kmers, missing, rows), name
        assert probe(acc, s, query, runs=False) == (kmers, missing), name
        s.close()
    names = [n for n, _ in acc.last_timing()]
    assert "kq_query" in names and "kq_insert" not in names


@pytest.mark.parametrize("k", kc.KS)
def test_full_tables_and_overflow(acc, k):
    e = expected(k)
    for name in ("two_batches", "tile_lengths", "tandem_repeat", "short_contigs"):
        truth, query, st, kmers, missing, rows = e[name]
        s = build(acc, k, st[1], truth)                      # load 1.0: chains that wrap, absent keys walk the whole table
        assert s.stats == st + (st[1],) and probe(acc, s, query) == (kmers, missing, rows), name
        s.close()
        for slots in (st[1] - 1, 1):                         # a table that is too small is a status, never a hang
            with pytest.raises(cornetto_amd.AccelError) as ei:
                build(acc, k, slots, truth)
            assert ei.value.status == kc.E_NOMEM, (name, slots)
    truth, query, st, kmers, missing, rows = e["homopolymer"]
    s = build(acc, k, 1, truth)                              # every lane CASes the one slot
    assert st[1] == 1 and s.stats == st + (1,) and probe(acc, s, query) == (kmers, missing, rows)
    a = acc.asm_upload([kc.dna(__import__("random").Random(3), 200)])
    with pytest.raises(cornetto_amd.AccelError) as ei:
        s.add(a)
    assert ei.value.status == kc.E_NOMEM
    for call in (lambda: s.add(a), lambda: s.query(a)):      # the set is unusable from then on
        with pytest.raises(cornetto_amd.AccelError):
            call()
    a.close()
    s.close()


def test_batches_assemblies_in_turn_and_arguments(acc):
    k = 21
    truth, query, st, kmers, missing, rows = expected(k)["two_batches"]
    one = build(acc, k, 3 * st[0], [[s for b in truth for s in b]])
    two = build(acc, k, 3 * st[0], truth)
    assert one.stats == two.stats == st + (3 * st[0],)
    other = expected(k)["one_substitution"]
    for _ in range(2):                                       # the same set, two assemblies in turn
        for s in (one, two):
            assert probe(acc, s, query) == (kmers, missing, rows)
            S, _ = kc.truth_set([x for b in truth for x in b], k)
            assert probe(acc, s, other[1]) == kc.query(S, other[1], k)
    assert probe(acc, one, []) == ([], [], []) and probe(acc, one, [b"", b"ACGT"]) == ([0, 0], [0, 0], [])
    one.close()
    two.close()
    for bad_k in (9, 10, 20, 32, 33, 0, -1):
        with pytest.raises(cornetto_amd.AccelError) as ei:
            acc.kset(bad_k, 10)
        assert ei.value.status == kc.E_UNSUPPORTED
    with pytest.raises(cornetto_amd.AccelError) as ei:
        acc.kset(21, 0)
    assert ei.value.status == -3
    with pytest.raises(cornetto_amd.AccelError) as ei:
        acc.kset(21, 1 << 46)                                # 512 TiB: the message says how many bytes were wanted
    assert ei.value.status == kc.E_NOMEM and str((1 << 46) * 8) in str(ei.value)


def test_nothing_depends_on_what_the_memory_held(dacc):
    """the table over memory that held 0x00 and then 0x5a (a freed block of the same size is what the next allocation usually gets), and the
    handle's workspaces — counters, bitmap, run words, rows — filled with both between two queries"""
    import torch
    import selftest_bind as st
    k = 21
    truth, query, stt, kmers, missing, rows = expected(k)["two_batches"]
    slots = 2 * stt[0] + 1
    for byte in (0x00, 0x5A):
        junk = torch.full((slots * 8,), byte, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        del junk
        torch.cuda.empty_cache()
        s = build(dacc, k, slots, truth)
        assert s.stats == stt + (slots,) and probe(dacc, s, query) == (kmers, missing, rows), byte
        filled, _, _ = st.ws_fill(dacc, byte)
        assert {"WS_KQ_CNT", "WS_KQ_MAP", "WS_KQ_ROWS"} <= set(filled)
        assert probe(dacc, s, query) == (kmers, missing, rows), byte
        st.ws_fill(dacc, 0xFF)
        assert probe(dacc, s, query[:1]) == (kmers[:1], missing[:1], [r for r in rows if r[0] == 0]), byte
        assert probe(dacc, s, query) == (kmers, missing, rows), byte
        s.close()


def test_moderate(acc):
    truth, q = kc.moderate(21)
    S, n_pos = kc.truth_set(truth, 21)
    s = build(acc, 21, 2 * n_pos, [truth[:4], truth[4:]])
    assert s.stats == (n_pos, len(S), 2 * n_pos)
    kmers, missing, rows = kc.query(S, q, 21)
    assert sum(missing) > 1000 and len(rows) > 100
    assert probe(acc, s, q) == (kmers, missing, rows)
    s.close()


@pytest.mark.parametrize("k", kc.KS)
def test_cli_device_and_host_print_the_same_bytes(tmp_path, k):
    """every case of k in one truth (a plain file and a gzip -t file) and one assembly: the device's bytes, the host path's and the formatter's"""
    e = expected(k)
    t0 = [("t%d" % i, s) for i, s in enumerate(s for n in sorted(e) for s in e[n][0][0])]
    t1 = [("u%d" % i, s) for i, s in enumerate(s for n in sorted(e) for b in e[n][0][1:] for s in b)]
    q = [("q%d" % i, s) for i, s in enumerate(s for n in sorted(e) for s in e[n][1])]
    (tmp_path / "t0.fa").write_bytes(kc.fasta(t0, width=60))
    (tmp_path / "t1.fa.gz").write_bytes(gzip.compress(kc.fasta(t1)))
    (tmp_path / "q.fa").write_bytes(kc.fasta(q, width=80))
    apath = str(tmp_path / "q.fa")
    w = kc.expect_cli([t0, t1], [(apath, q)], k)
    for mode in ("dev", "host"):
        args = [cornetto_amd.CLI_PATH, "qv", "-k", str(k), "-t", str(tmp_path / "t1.fa.gz"), "-c", str(tmp_path / (mode + ".tsv")), "-b", str(tmp_path / (mode + ".bed"))]
        p = subprocess.run(args + (["--accel=no"] if mode == "host" else []) + [str(tmp_path / "t0.fa"), apath], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and p.stdout == w["stdout"], (mode, p.stderr[-2000:])
        assert (tmp_path / (mode + ".tsv")).read_bytes() == w["contigs"] and (tmp_path / (mode + ".bed")).read_bytes() == w["bed"], mode
        assert [ln for ln in p.stderr.split(b"\n") if ln.startswith(b"[qv]")] == [w["truth_line"]], mode
    if k == 21:      # two assemblies in argument order; a table that is too small: one ERROR line that names --slots, nothing on stdout
        w2 = kc.expect_cli([t0], [(apath, q), (str(tmp_path / "t0.fa"), t0)], k)
        p = subprocess.run([cornetto_amd.CLI_PATH, "qv", str(tmp_path / "t0.fa"), apath, str(tmp_path / "t0.fa")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and p.stdout == w2["stdout"], p.stderr[-2000:]
        p = subprocess.run([cornetto_amd.CLI_PATH, "qv", "--slots", str(w2["distinct"] - 1), str(tmp_path / "t0.fa"), apath], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        lines = [ln for ln in p.stderr.split(b"\n") if b"ERROR" in ln]
        assert p.returncode == 1 and p.stdout == b"" and len(lines) == 1 and b"--slots" in lines[0], p.stderr[-2000:]
