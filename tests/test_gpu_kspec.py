"""GPU: the copies of an assembly and the copy-number spectrum of a counted k-mer set (csrc/kcount.hip: kq_copies, kq_spectrum) against the two
Counters of tests/kspec_cases.py: exact equality of the 6 x 1024 spectrum, of solid and found for every threshold, of the set's stats, histogram,
seal and later probes, through the binding; the state machine's refusals; copies over memory that held other bytes; and the bytes of
`qv -r --completeness --spectra-cn` on the device and with --accel=no.  The cases are the smallest shapes at which the kernels can go wrong, each
for k = 11, 21 and 31; the expected values are computed once per k and shared."""
import subprocess

import numpy as np
import pytest

import cornetto_amd
import kcount_cases as cc
import kqv_cases as kc
import kspec_cases as ks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def names(acc):
    return [n for n, _ in acc.last_timing()]


def raises(status, call):
    with pytest.raises(cornetto_amd.AccelError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return str(ei.value)


def counted(acc, k, slots, reads):
    s = acc.kset(k, slots, channels=1)
    for b in reads:
        a = acc.asm_upload(b)
        s.count(a)
        a.close()
    return s


def copies(acc, s, batches):
    for b in batches:
        a = acc.asm_upload(b)
        s.copies(a)
        assert names(acc) == (["kq_copies"] if sum(map(len, b)) else []), names(acc)
        a.close()


def spectrum(acc, s, m):
    spec, solid, found = s.spectrum(m)
    assert names(acc) == ["kq_spectrum"] and spec.shape == (ks.CN, ks.BINS) and spec.dtype == np.int64
    return spec.tolist(), (solid, found)


@pytest.mark.parametrize("k", ks.KS)
def test_cases(acc, k):
    for name, e in ks.expected(k).items():
        slots = ks.slots_of(e)
        s = counted(acc, k, slots, e.case.reads)
        st = s.stats
        assert st == e.stats + (slots,), name
        hist = s.hist().tolist()
        assert hist == e.hist, name
        # before any copy: row 0 is the histogram, and solid is what the seal will say
        spec, tot = spectrum(acc, s, e.case.ms[0])
        assert spec[0] == hist and not any(map(any, spec[1:])) and tot == (e.totals[e.case.ms[0]][0], 0), name
        copies(acc, s, e.case.asm)
        for m in e.case.ms:
            assert spectrum(acc, s, m) == (e.spec, e.totals[m]), (name, m)
        spec = np.array(e.spec)
        assert spec[:, 1:].sum(0).tolist() == hist[1:] and spec[0, 0] == 0, name
        # the copies have moved neither the stats nor the histogram, and the seal returns solid
        assert s.stats == st and s.hist().tolist() == hist, name
        assert s.seal(e.case.ms[-1]) == (e.totals[e.case.ms[-1]][0],) and s.stats == st, name
        s.close()


@pytest.mark.parametrize("k", ks.KS)
def test_two_assemblies_and_the_clear(acc, k):
    p, B = ks.expected(k)["planted"], ks.second_assembly(k)
    R, _ = ks.counter(p.case.reads, k)
    Bc, _ = ks.counter(B, k)
    want_b = (ks.spectrum(R, Bc), ks.totals(R, Bc, 2))
    slots = ks.slots_of(p) + 1000
    s = counted(acc, k, slots, p.case.reads)
    s.copies_clear()                                           # nothing to clear yet: accepted
    copies(acc, s, p.case.asm)
    assert spectrum(acc, s, 2) == (p.spec, p.totals[2])
    s.copies_clear()
    spec, tot = spectrum(acc, s, 2)                            # A's assembly-only keys are still in the table, in no cell
    assert spec[0] == p.hist and not any(map(any, spec[1:])) and tot == (p.totals[2][0], 0)
    copies(acc, s, B)
    assert spectrum(acc, s, 2) == want_b and want_b[0][0][0] == 0
    s.copies_clear()
    copies(acc, s, p.case.asm[::-1])
    assert spectrum(acc, s, 2) == (p.spec, p.totals[2])
    s.close()
    fresh = counted(acc, k, slots, p.case.reads)
    copies(acc, fresh, B)
    assert spectrum(acc, fresh, 2) == want_b
    fresh.close()


@pytest.mark.parametrize("k", ks.KS)
def test_the_seal_and_the_probes_are_unchanged(acc, k):
    """after copies calls with assembly-only keys the set seals into what it would have sealed into without them"""
    for name in ("multiplicity", "tombstones_at_load_1", "short_reads"):
        case, st, hists, by_m = cc.expected(k)[name]
        novel = [kc.dna(__import__("random").Random(k), 700)]
        R, _ = ks.counter([b for _, b in case.reads], k)
        A, _ = ks.counter([case.query, novel], k)
        slots = len(set(R) | set(A)) if case.slots else cc.slots_of(case, st) + 2000
        for m in case.ms:
            s = counted(acc, k, slots, [b for _, b in case.reads])
            copies(acc, s, [case.query, novel])
            assert spectrum(acc, s, m[0]) == (ks.spectrum(R, A), ks.totals(R, A, m[0])), (name, m)
            s.copies_clear()
            copies(acc, s, [novel])
            assert s.stats == st + (slots,) and s.hist().tolist() == hists[0], (name, m)
            solid, want = by_m[m]
            assert s.seal(m) == solid and names(acc) == ["kq_seal"] and s.stats == st + (slots,), (name, m)
            a = acc.asm_upload(case.query)
            r = s.query(a, runs=True)
            a.close()
            assert (list(map(int, r[0])), list(map(int, r[1])), [tuple(map(int, x)) for x in r[2]]) == tuple(want), (name, m)
            s.close()


@pytest.mark.parametrize("k", ks.KS)
def test_a_table_too_small_is_a_status_and_the_set_is_dead(acc, k):
    e = ks.expected(k)["neighbours_at_load_1"]
    a = acc.asm_upload(e.case.asm[0])
    for slots in (e.union - 1, e.stats[1]):
        s = counted(acc, k, slots, e.case.reads)
        raises(ks.E_NOMEM, lambda: s.copies(a))
        raises(ks.E_NOMEM, lambda: s.copies(a))
        for call in (lambda: s.spectrum(1), lambda: s.copies_clear(), lambda: s.hist(), lambda: s.seal(2), lambda: s.count(a), lambda: s.query(a)):
            with pytest.raises(cornetto_amd.AccelError):
                call()
        s.close()
    a.close()
    # the reads' distinct keys are enough for an assembly that holds only read k-mers
    s = counted(acc, k, e.stats[1], e.case.reads)
    copies(acc, s, [e.case.reads[0][:1]])
    spec, tot = spectrum(acc, s, 1)
    assert tot[0] == e.stats[1] and 0 < tot[1] <= tot[0] and not any(spec[a][0] for a in range(ks.CN))
    s.close()


def test_the_state_machine_refuses_calls_out_of_order(acc):
    k = 21
    e = ks.expected(k)["seams"]
    a = acc.asm_upload(e.case.asm[0])
    plain = acc.kset(k, 100000)
    for call in (lambda: plain.copies(a), lambda: plain.copies_clear(), lambda: plain.spectrum(1)):
        raises(ks.E_UNSUPPORTED, call)
    plain.add(a)
    raises(ks.E_UNSUPPORTED, lambda: plain.copies(a))
    plain.close()
    tagged = acc.kset(k, 100000)
    tagged.add(a, tag=1)
    two = acc.kset(k, 100000, channels=2)
    two.count(a, 1)
    for s in (tagged, two):
        for call in (lambda: s.copies(a), lambda: s.copies_clear(), lambda: s.spectrum(1), lambda: s.spectrum(1, channel=1)):
            raises(ks.E_UNSUPPORTED, call)
        s.close()
    s = counted(acc, k, ks.slots_of(e), e.case.reads)
    for bad in (0, -1, ks.CAP + 1):
        raises(ks.E_ARG, lambda: s.spectrum(bad))
    for ch in (-1, 1):
        raises(ks.E_ARG, lambda: s.spectrum(1, channel=ch))
    s.count(a)                                                  # still a counted set that takes counts ...
    s.copies(a)
    raises(ks.E_UNSUPPORTED, lambda: s.count(a))                # ... until its first copies call
    s.copies_clear()
    raises(ks.E_UNSUPPORTED, lambda: s.count(a))                # the keys stay
    assert s.spectrum(ks.CAP)[1:] == (0, 0)
    s.seal(1)
    for call in (lambda: s.copies(a), lambda: s.copies_clear(), lambda: s.spectrum(1)):
        raises(ks.E_UNSUPPORTED, call)
    assert s.query(a)[1].sum() == 0
    s.close()
    a.close()


def test_nothing_depends_on_what_the_memory_held(dacc):
    """the copies allocated over memory that held 0x5a (a freed block of the same size is what the next allocation usually gets), and the handle's
    workspaces — the spectrum's among them — filled between two spectrum calls"""
    import torch
    import selftest_bind as st
    k = 21
    e = ks.expected(k)["seams"]
    slots = ks.slots_of(e)
    for byte in (0x5A, 0xFF):
        s = counted(dacc, k, slots, e.case.reads)
        junk = [torch.full(((slots + 3) // 4 * 4,), byte, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        del junk
        torch.cuda.empty_cache()
        copies(dacc, s, e.case.asm)
        assert spectrum(dacc, s, 2) == (e.spec, e.totals[2]), byte
        filled, _, _ = st.ws_fill(dacc, byte)
        assert "WS_KC_HIST" in filled
        assert spectrum(dacc, s, 2) == (e.spec, e.totals[2]) and s.hist().tolist() == e.hist, byte
        st.ws_fill(dacc, 0x00)
        assert spectrum(dacc, s, 1) == (e.spec, e.totals[1]), byte
        s.close()


@pytest.mark.parametrize("k", ks.KS)
def test_cli_device_and_host_print_the_same_bytes(tmp_path, k):
    exp = ks.expected(k)
    named = lambda seqs, tag: [("%s%d" % (tag, i), s) for i, s in enumerate(seqs)]          # noqa: E731
    p, sm = exp["planted"].case, exp["seams"].case
    r0, r1 = named(p.reads[0] + [s for s in sm.reads[0] if s], "a"), named(p.reads[1], "b")
    qa, qb = named(p.asm[0] + sm.asm[0], "q"), named(ks.second_assembly(k)[0], "w")
    (tmp_path / "r0.fq").write_bytes(cc.fastq(r0))
    (tmp_path / "r1.fa").write_bytes(kc.fasta(r1))
    (tmp_path / "qa.fa").write_bytes(kc.fasta(qa, width=80))
    (tmp_path / "qb.fa").write_bytes(kc.fasta(qb))
    pa, pb = str(tmp_path / "qa.fa"), str(tmp_path / "qb.fa")
    rd = ["-r", str(tmp_path / "r0.fq"), "-r", str(tmp_path / "r1.fa")]

    def cli(args, host):
        return subprocess.run([cornetto_amd.CLI_PATH, "qv"] + (["--accel=no"] if host else []) + ["-k", str(k)] + rd + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for m in (2, 1024):
        w = ks.expect_qv([r0, r1], [(pa, qa)], k, m)
        w2 = ks.expect_qv([r0, r1], [(pb, qb), (pa, qa), (pb, qb)], k, m)
        for host in (False, True):
            f = str(tmp_path / ("s%d.tsv" % host))
            r = cli(["--min-count", str(m), "--completeness", "--spectra-cn", f, pa], host)
            assert r.returncode == 0 and r.stdout == w["stdout"] and open(f, "rb").read() == w["spectra"], (host, m, r.stderr[-2000:])
            assert [ln for ln in r.stderr.split(b"\n") if ln.startswith(b"[qv]")] == [w["line"]], (host, m)
            r = cli(["--min-count", str(m), "--completeness", pb, pa, pb], host)
            assert r.returncode == 0 and r.stdout == w2["stdout"], (host, m, r.stderr[-2000:])
            r = cli(["--min-count", str(m), pa], host)
            assert r.returncode == 0 and r.stdout == w["plain"], (host, m)
    if k == 21:      # the assembly-only k-mers find no slot: one ERROR line that names --slots, nothing on stdout
        r = cli(["--slots", str(w["union"] - 1), "--completeness", pa], False)
        lines = [ln for ln in r.stderr.split(b"\n") if b"ERROR" in ln]
        assert r.returncode == 1 and r.stdout == b"" and len(lines) == 1 and b"--slots" in lines[0], r.stderr[-2000:]
        r = cli(["--slots", str(w["union"]), "--min-count", "2", "--completeness", pa], False)
        assert r.returncode == 0 and r.stdout == ks.expect_qv([r0, r1], [(pa, qa)], k, 2)["stdout"], r.stderr[-2000:]
