"""GPU: the counted k-mer set (csrc/kcount.hip) against the Counter of tests/kcount_cases.py: exact equality of stats, histogram, solid counts and of
what the old probes (kq_query, kt_mark / kt_tile / kt_seam) answer on the sealed set, through the binding; the state machine's refusals; a table
over memory that held other bytes; and the bytes of `qv -r` and `trioeval --pat-reads --mat-reads` on the device and with --accel=no.  The cases
are the smallest shapes at which the kernels can go wrong, each for k = 11, 21 and 31; the expected values are computed once per k and shared."""
import gzip
import subprocess

import pytest

import cornetto_amd
import kcount_cases as cc
import kqv_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def fill(acc, k, slots, case, upto=None):
    s = acc.kset(k, slots, channels=case.channels)
    for ch, b in case.reads[:upto]:
        a = acc.asm_upload(b)
        s.count(a, ch)
        a.close()
    return s


def probe(acc, s, case):
    a = acc.asm_upload(case.query)
    if case.channels == 1:
        r = s.query(a, runs=True)
        out = (list(map(int, r[0])), list(map(int, r[1])), [tuple(map(int, x)) for x in r[2]])
    else:
        out = [list(map(int, row)) for row in s.phase(a)]
    a.close()
    return out


def names(acc):
    return [n for n, _ in acc.last_timing()]


def raises(status, call):
    with pytest.raises(cornetto_amd.AccelError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return str(ei.value)


@pytest.mark.parametrize("k", cc.KS)
def test_cases(acc, k):
    for name, (case, st, hists, by_m) in cc.expected(k).items():
        slots = cc.slots_of(case, st)
        for m in case.ms:
            s = fill(acc, k, slots, case)
            assert names(acc) == ["kq_count"] and s.stats == st + (slots,), (name, m)
            for ch in range(case.channels):
                assert s.hist(ch).tolist() == hists[ch] and names(acc) == ["kq_hist"], (name, m, ch)
            solid, want = by_m[m]
            assert s.seal(m) == solid and names(acc) == ["kq_seal"] and s.stats == st + (slots,), (name, m)
            for _ in range(2):
                assert probe(acc, s, case) == (want if case.channels == 2 else tuple(want)), (name, m)
            # the probes are the old kernels
            assert names(acc)[:1] == (["kq_query"] if case.channels == 1 else ["kt_mark"]) and "kq_count" not in names(acc), (name, m)
            s.close()


@pytest.mark.parametrize("k", cc.KS)
def test_a_table_too_small_is_a_status_and_the_set_is_dead(acc, k):
    case, st, hists, by_m = cc.expected(k)["tombstones_at_load_1"]
    a = acc.asm_upload(case.query)
    for slots in (st[1] - 1, 1):
        s = acc.kset(k, slots, channels=1)
        b = acc.asm_upload(case.reads[0][1])
        raises(cc.E_NOMEM, lambda: s.count(b))
        raises(cc.E_NOMEM, lambda: s.count(b))
        for call in (lambda: s.hist(), lambda: s.seal(2), lambda: s.query(a), lambda: s.add(b)):
            with pytest.raises(cornetto_amd.AccelError):
                call()
        b.close()
        s.close()
    a.close()
    # one key in one slot: every lane of every wave walks to the same slot and adds to the same count
    case, st, hists, by_m = cc.expected(k)["cap_and_last_bin"]
    s = fill(acc, k, 2, case, upto=1)
    h = s.hist()
    assert h[1023] == 1 and h.sum() == 1 and s.stats == (17 * cc.TILE - k + 1, 1, 2)
    s.close()
    s = fill(acc, k, 1, case, upto=1)
    assert s.seal(cc.CAP) == (1,) and probe(acc, s, case)[1][:2] == [0, 50 - k + 1]
    s.close()


def test_the_state_machine_refuses_calls_out_of_order(acc):
    k = 21
    case, st, hists, by_m = cc.expected(k)["multiplicity"]
    a = acc.asm_upload(case.query)
    plain = acc.kset(k, 1000)
    for call in (lambda: plain.count(a), lambda: plain.hist(), lambda: plain.seal(1)):
        raises(cc.E_UNSUPPORTED, call)
    plain.close()
    for channels in (1, 2):
        s = acc.kset(k, 4 * st[0], channels=channels)
        s.count(a, channels - 1)
        for call in (lambda: s.add(a), lambda: s.add(a, tag=1), lambda: s.query(a), lambda: s.phase(a)):      # not before the seal, the adds never
            raises(cc.E_UNSUPPORTED, call)
        for ch in (-1, channels):
            raises(cc.E_ARG, lambda: s.count(a, ch))
            raises(cc.E_ARG, lambda: s.hist(ch))
        for bad in (0, -1, cc.CAP + 1):
            raises(cc.E_ARG, lambda: s.seal([bad] * channels))
            raises(cc.E_ARG, lambda: s.seal([1] * (channels - 1) + [bad]))
        assert s.hist(channels - 1).sum() == s.stats[1] > 0          # the refused seals have changed nothing
        assert s.seal([1] * channels)[channels - 1] == s.stats[1]
        for call in (lambda: s.seal([1] * channels), lambda: s.count(a, 0), lambda: s.hist(0), lambda: s.add(a), lambda: s.add(a, tag=2)):
            raises(cc.E_UNSUPPORTED, call)
        if channels == 1:
            raises(cc.E_UNSUPPORTED, lambda: s.phase(a))
            assert s.query(a)[1].sum() == 0
        else:
            raises(cc.E_UNSUPPORTED, lambda: s.query(a))
            assert s.phase(a)[:, 1].sum() == 0 and s.phase(a)[:, 2].sum() == s.phase(a)[:, 0].sum() > 0      # every k-mer is the mother's alone
        s.close()
    a.close()
    raises(cc.E_ARG, lambda: acc.kset(k, 10, channels=3))
    raises(cc.E_ARG, lambda: acc.kset(k, 10, channels=-1))
    raises(cc.E_ARG, lambda: acc.kset(k, 0, channels=1))
    raises(cc.E_UNSUPPORTED, lambda: acc.kset(20, 10, channels=1))
    for channels in (1, 2):      # the message says how many bytes were wanted: 12 and 16 per slot
        assert str((1 << 46) * (8 + 4 * channels)) in raises(cc.E_NOMEM, lambda: acc.kset(k, 1 << 46, channels=channels))


def test_nothing_depends_on_what_the_memory_held(dacc):
    """the table and the counts over memory that held 0x00 and then 0x5a (a freed block of the same size is what the next allocation usually
    gets), and the handle's workspaces — the histogram among them — filled with both between two hist calls and between two probes"""
    import torch
    import selftest_bind as st
    k = 21
    for name in ("short_reads", "two_channels"):
        case, stt, hists, by_m = cc.expected(k)[name]
        slots = cc.slots_of(case, stt)
        m = case.ms[0]
        for byte in (0x00, 0x5A):
            junk = [torch.full((slots * n,), byte, dtype=torch.uint8, device="cuda") for n in (8, 4 * case.channels)]
            torch.cuda.synchronize()
            del junk
            torch.cuda.empty_cache()
            s = fill(dacc, k, slots, case)
            assert s.stats == stt + (slots,) and s.hist(0).tolist() == hists[0], (name, byte)
            filled, _, _ = st.ws_fill(dacc, byte)
            assert "WS_KC_HIST" in filled
            assert [s.hist(ch).tolist() for ch in range(case.channels)] == hists, (name, byte)
            assert s.seal(m) == by_m[m][0], (name, byte)
            want = by_m[m][1] if case.channels == 2 else tuple(by_m[m][1])
            assert probe(dacc, s, case) == want, (name, byte)
            st.ws_fill(dacc, 0xFF)
            assert probe(dacc, s, case) == want, (name, byte)
            s.close()


def cli_run(args, host):
    p = subprocess.run([cornetto_amd.CLI_PATH] + args[:1] + (["--accel=no"] if host else []) + args[1:], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p


@pytest.mark.parametrize("k", cc.KS)
def test_cli_device_and_host_print_the_same_bytes(tmp_path, k):
    """one plain and one gzip reads file per command: the device's bytes, the host path's and the formatter's"""
    e = cc.expected(k)
    case = e["short_reads"][0]
    r0 = [("a%d" % i, s) for i, s in enumerate(case.reads[0][1] + e["multiplicity"][0].reads[0][1])]
    r1 = [("b%d" % i, s) for i, s in enumerate(case.reads[1][1])]
    q = [("q%d" % i, s) for i, s in enumerate(case.query + e["multiplicity"][0].query)]
    (tmp_path / "r0.fq").write_bytes(cc.fastq([r for r in r0 if r[1]]))
    r0 = [r for r in r0 if r[1]]
    (tmp_path / "r1.fa.gz").write_bytes(gzip.compress(kc.fasta(r1)))
    (tmp_path / "q.fa").write_bytes(kc.fasta(q, width=80))
    apath = str(tmp_path / "q.fa")
    for m in (2, 1):
        w = cc.expect_qv([r0, r1], [(apath, q)], k, m)
        for mode in ("dev", "host"):
            f = dict((x, str(tmp_path / (mode + x))) for x in (".tsv", ".bed", ".hist"))
            p = cli_run(["qv", "-k", str(k), "-r", str(tmp_path / "r0.fq"), "-r", str(tmp_path / "r1.fa.gz"), "--min-count", str(m), "--hist", f[".hist"], "-c", f[".tsv"],
                         "-b", f[".bed"], apath], mode == "host")
            assert p.returncode == 0 and p.stdout == w["stdout"], (mode, m, p.stderr[-2000:])
            assert [open(f[x], "rb").read() for x in (".tsv", ".bed", ".hist")] == [w["contigs"], w["bed"], w["hist"]], (mode, m)
            assert [ln for ln in p.stderr.split(b"\n") if ln.startswith(b"[qv]")] == [w["line"]], (mode, m)
    case = e["mosaic_twice"][0]
    two = e["two_channels"][0]
    pat = [("p%d" % i, s) for i, s in enumerate(s for ch, b in case.reads + two.reads if ch == 0 for s in b)]
    mat = [("m%d" % i, s) for i, s in enumerate(s for ch, b in case.reads + two.reads if ch == 1 for s in b)]
    q = [("q%d" % i, s) for i, s in enumerate(case.query + two.query)]
    (tmp_path / "pat.fq.gz").write_bytes(gzip.compress(cc.fastq(pat)))
    (tmp_path / "mat.fa").write_bytes(kc.fasta(mat, width=60))
    (tmp_path / "q2.fa").write_bytes(kc.fasta(q, width=80))
    apath = str(tmp_path / "q2.fa")
    for m in ((2, 2), (1, 2)):
        w = cc.expect_trio([pat], [mat], [(apath, q)], k, m)
        for mode in ("dev", "host"):
            f = dict((x, str(tmp_path / (mode + x))) for x in (".tsv", ".hist"))
            p = cli_run(["trioeval", "-k", str(k), "--pat-reads", str(tmp_path / "pat.fq.gz"), "--mat-reads", str(tmp_path / "mat.fa"), "--min-count", "%d,%d" % m,
                         "--hist", f[".hist"], "-c", f[".tsv"], apath], mode == "host")
            assert p.returncode == 0 and p.stdout == w["stdout"], (mode, m, p.stderr[-2000:])
            assert [open(f[x], "rb").read() for x in (".tsv", ".hist")] == [w["contigs"], w["hist"]], (mode, m)
            assert [ln for ln in p.stderr.split(b"\n") if ln.startswith(b"[trioeval]")] == [w["line"]], (mode, m)
    if k == 21:      # a table that is too small: one ERROR line that names --slots, nothing on stdout
        p = cli_run(["trioeval", "--slots", str(w["distinct"] - 1), "--pat-reads", str(tmp_path / "pat.fq.gz"), "--mat-reads", str(tmp_path / "mat.fa"), apath], False)
        lines = [ln for ln in p.stderr.split(b"\n") if b"ERROR" in ln]
        assert p.returncode == 1 and p.stdout == b"" and len(lines) == 1 and b"--slots" in lines[0], p.stderr[-2000:]
