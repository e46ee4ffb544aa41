"""GPU: cornetto_telo_ends() (Accel.telo_ends) and `cornetto telostats` on the device path against the restatement of scripts/telostats.sh
in tests/telostats_cases.py.  The planted cases put regions where the device stage changes path — the seam between two window tiles (window
index 255|256 = base 51 200), gaps of exactly G and G + 1 windows across it, the clipped final window, the lengths at which the window loop
and the end intervals change, a bordered motif (the marks come from the runs, not from tf_scan), long motifs — and every one asserts on the
expected data that it has the property it is named after.  Then 150 random small assemblies, the CLI under its input routes against the
host path byte for byte, a 20 Mbase assembly, two calls with different merge distances on one handle, and a call whose region list was
sized too small."""
import hashlib
import os

import numpy as np
import pytest

import cornetto_amd
import telostats_cases as tc
from helpers import read_fastx

pytestmark = pytest.mark.gpu

SEAM = 256 * 200      # the first base of the second window tile of a record


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def device_rows(acc, records, m=b"TTAGGG", t=0.4, I=99.9, d=100, E=50000):
    asm = acc.asm_upload([r[1] for r in records])
    try:
        rows = acc.telo_ends(asm, m, acc.telowin_threshold(t, I), d, E)
        return [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in rows]
    finally:
        asm.close()


def qual_indices(seq, **kw):
    return [s // 200 for s, _ in tc.windows(seq, **kw)]


# ---- the planted cases: name -> (records, parameters, property of the expected data) ----------------------------------------------------
def gap_case(d, extra):
    """two blocks of 402 telomeric bases at window starts: the first qualifies windows J0 - 3 .. J0 = 253, the second J1 - 3 .. J1; the gap
    between window 253 and window J1 - 3 is G + extra windows, across the tile seam"""
    G = (1000 + d) // 200
    j0, j1 = 253, 253 + G + extra + 3
    L = 200 * j1 + 5000
    rec = (b"gap", tc.planted(np.random.default_rng(21), L, [(200 * j0, 200 * j0 + 402), (200 * j1, 200 * j1 + 402)]))

    def prop(exp):
        q = qual_indices(rec[1])
        pairs = [(a, b) for a, b in zip(q, q[1:]) if a <= 255 < b]
        assert pairs == [(253, 253 + G + extra)], (q, G)
        assert len(exp["regions"][0]) == (1 if extra == 0 else 2)
    return [rec], {"d": d, "E": L}, prop


def planted_cases():
    rng = np.random.default_rng(20)
    cases = {}

    rec = (b"seam", tc.planted(rng, 60000, [(50000, 52600)]))
    def prop_seam(exp):
        (s, e), = exp["regions"][0]
        assert s // 200 <= 255 and (e - 1000) // 200 >= 256 and s < SEAM < e
    cases["region_across_the_tile_seam"] = ([rec], {"E": 30000}, prop_seam)

    for d in (100, 0, 1000, 11799):
        cases["gap_G_d%d" % d] = gap_case(d, 0)
        cases["gap_G_plus_1_d%d" % d] = gap_case(d, 1)

    L = 10333
    rec = (b"clip", tc.planted(rng, L, [(8300, L)]))
    def prop_clip(exp, L=L, rec=rec):
        s, e = exp["regions"][0][-1]
        last = 200 * (tc.visited(L) - 1)
        assert e == L and L - last < 1000 and (last, L) in tc.windows(rec[1])
    cases["last_window_clipped"] = ([rec], {"E": 2000}, prop_clip)

    E = 30000
    lens = [0, 1, 999, 1000, 1001, 51200, 51201, 2 * E, 2 * E + 1]
    recs = [(b"len%d" % n, tc.telomere(n)) for n in lens]
    def prop_lens(exp):
        assert exp["c"] == [0, 0, 1, 1, 1, 1, 1, 1, 2], exp["c"]
        assert exp["regions"][5] == [(0, 51200)] and exp["regions"][6] == [(0, 51201)]
    cases["record_lengths"] = (recs, {"E": E}, prop_lens)
    recs2 = [(b"bg%d" % n, tc.planted(rng, n, [(max(0, n - 1300), n)])) for n in lens]
    def prop_lens2(exp):
        assert exp["c"][0] == 0 and all(c >= 1 for c in exp["c"][2:]) and exp["regions"][6][-1][1] == 51201
    cases["record_lengths_telomere_at_the_end"] = (recs2, {"E": E}, prop_lens2)

    rec = (b"whole", tc.telomere(2 * E + 200))
    def prop_whole(exp):
        assert exp["regions"][0] == [(0, 2 * E + 200)] and exp["rows"] == [(0, 0, 2 * E + 200)] * 2 and (exp["one"], exp["two"], exp["more"]) == (0, 1, 0)
    cases["fully_telomeric_record"] = ([rec], {"E": E}, prop_whole)

    L = 30000
    rec = (b"touch", tc.planted(rng, L, [(10000, 11400), (20600, 22000)]))
    (s1, e1), (s2, e2) = tc.merge(tc.windows(rec[1]), 100)
    for name, Et, want in (("left_end_by_0_bases", s1, [(s2, e2)]), ("left_end_by_1_base", s1 + 1, [(s1, e1), (s2, e2)]),
                           ("right_end_by_0_bases", L - e2, []), ("right_end_by_1_base", L - e2 + 1, [(s2, e2)])):
        def prop_touch(exp, Et=Et, want=want, L=L):
            assert L > 2 * Et and exp["regions"][0] == [(s1, e1), (s2, e2)] and [(s, e) for _, s, e in exp["rows"]] == want
        cases["region_touches_the_" + name] = ([rec], {"E": Et}, prop_touch)

    recs = [(b"a", tc.planted(rng, 8000, [(0, 1500)])), (b"quiet", tc.background(rng, 5000)), (b"b", tc.planted(rng, 9000, [(7500, 9000)]))]
    def prop_quiet(exp, recs=recs):
        assert exp["c"] == [1, 0, 1] and not tc.windows(recs[1][1])
    cases["record_without_runs_between_two_with_runs"] = (recs, {"E": 2000}, prop_quiet)

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_selfoverlap.fa")
    recs = [(r[0], r[2]) for r in read_fastx(golden)] + [(b"acac", tc.planted(rng, 70000, [(0, 3000), (50900, 51500), (68000, 70000)], b"AC"))]
    def prop_bordered(exp):
        m = b"ACACA"
        assert any(m[:b] == m[-b:] for b in range(1, len(m)))           # a border: the greedy runs are not every match
        assert exp["c"][-1] == 2 and len(exp["regions"][-1]) == 3
    cases["bordered_motif"] = (recs, {"m": b"ACACA", "E": 5000}, prop_bordered)

    recs = [(b"a", tc.planted(rng, 60000, [(0, 2500), (50500, 52000)])), (b"b", tc.planted(rng, 9000, [(7500, 9000)], b"CCCTAA"))]
    def prop_long(exp):
        assert exp["c"] == [1, 1] and len(exp["regions"][0]) == 2
    cases["motif_of_12"] = (recs, {"m": b"TTAGGG" * 2, "E": 5000}, prop_long)
    cases["motif_of_36"] = (recs, {"m": b"TTAGGG" * 6, "E": 5000}, prop_long)
    return cases


CASES = planted_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_case(acc, name):
    records, kw, prop = CASES[name]
    exp = tc.expected(records, **kw)
    prop(exp)
    assert device_rows(acc, records, **kw) == exp["rows"]


@pytest.mark.parametrize("part", range(3))
def test_random_small_assemblies(acc, part):
    """150 assemblies of 1-6 records of 0-130 kb, random merge distance, ends and threshold"""
    rng = np.random.default_rng(900 + part)
    n_rows = 0
    for it in range(50):
        records = tc.random_assembly(rng)
        d = int(rng.choice([0, 1, 99, 100, 199, 200, 201, 999, 1000, 5000, 11799, int(rng.integers(0, 11800))]))
        E = int(rng.choice([1, 999, 5000, 50000, int(rng.integers(1, 70000))]))
        t = float(rng.choice([0.4, 0.4, 0.1, 0.05, 0.9, 1.0]))
        exp = tc.expected(records, b"TTAGGG", t, 99.9, d, E)
        assert device_rows(acc, records, t=t, d=d, E=E) == exp["rows"], (part, it, d, E, t)
        n_rows += len(exp["rows"])
    assert n_rows > 50


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("telostats_cli")
    rng = np.random.default_rng(33)
    records = [(b"both", tc.planted(rng, 120000, [(0, 3000), (50800, 51900), (117500, 120000)])), (b"none", tc.background(rng, 20000)), (b"empty", b""),
               (b"right", tc.planted(rng, 66001, [(64000, 66001)], b"CCCTAA")), (b"whole", tc.telomere(4200))]
    (d / "asm.fa").write_bytes(tc.fasta(records))
    (d / "asm.fq").write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in records))
    exp = tc.expected(records, E=2000)
    assert exp["c"] == [2, 0, 0, 1, 2]
    host = {}
    for f in ("asm.fa", "asm.fq"):
        hd = tmp_path_factory.mktemp("host")
        host[f] = tc.check_cli(cli, records, str(d / f), str(hd), tc.HOST, ["-e", "2000"], E=2000, exp=exp)
    return records, d, exp, host


@pytest.mark.parametrize("fname", ["asm.fa", "asm.fq"])
@pytest.mark.parametrize("env", [{}, {"CORNETTO_CLI_WHOLE": "0"}, {"CORNETTO_FASTQ_PIECE": "4096"}, {"CORNETTO_BATCH_BASES": "30000"},
                                 {"CORNETTO_BATCH_BASES": "30000", "CORNETTO_FASTQ_SPLIT": "host"}, {"CORNETTO_DEVICES": "0,0"}],
                         ids=["whole", "pieces", "small_pieces", "small_batches", "sequential_small_batches", "first_listed_device"])
def test_cli_routes(cli, cli_case, tmp_path, env, fname):
    records, d, exp, host = cli_case
    got = tc.check_cli(cli, records, str(d / fname), str(tmp_path), env, ["-e", "2000"], E=2000, exp=exp)
    assert got == host[fname]


def test_cli_golden_inputs(cli, golden_dir, tmp_path):
    for name, opts, kw in (("mix.fa.gz", ["-e", "300", "-t", "0.1"], {"E": 300, "t": "0.1"}), ("probe.fa", [], {}),
                           ("probe_selfoverlap.fa", ["-m", "ACACA", "-t", "0.01", "-e", "10"], {"m": b"ACACA", "t": "0.01", "E": 10})):
        path = os.path.join(golden_dir, name)
        records = [(r[0], r[2]) for r in read_fastx(path)]
        assert tc.check_cli(cli, records, path, str(tmp_path), {}, opts, **kw) == tc.check_cli(cli, records, path, str(tmp_path), tc.HOST, opts, **kw)


def test_the_device_path_is_taken(cli, cli_case, tmp_path):
    """CORNETTO_DEVICE names a device that does not exist: exit 1 and no BED rows (no silent host fallback)"""
    records, d, exp, host = cli_case
    got = tc.run_cli(cli, ["telostats", "-e", "2000", "-b", "out.bed", str(d / "asm.fa")], str(tmp_path), {"CORNETTO_DEVICE": "999"})
    assert got["rc"] == 1 and b"cannot open HIP device" in got["err"] and b"total telomere regions" not in got["out"]
    assert not os.path.exists(tmp_path / "out.bed") or os.path.getsize(tmp_path / "out.bed") == 0


def test_unsupported_merge_distance(acc):
    asm = acc.asm_upload([tc.telomere(3000)])
    for d in (-1, 11800):
        with pytest.raises(cornetto_amd.AccelError) as e:
            acc.telo_ends(asm, b"TTAGGG", 0.4, d, 1000)
        assert e.value.status == -5
    assert len(acc.telo_ends(asm, b"TTAGGG", 0.4, 11799, 1000)) == 2
    asm.close()


def test_assembly_of_20_mbases(cli, tmp_path):
    """30 contigs, telomeric ends planted on some: the device path, the host path and the restatement agree (sha256 of the BED)"""
    rng = np.random.default_rng(44)
    records = []
    for i in range(30):
        L = int(rng.integers(300_000, 1_050_000))
        blocks = ([(0, int(rng.integers(800, 9000)))] if i % 3 != 1 else []) + ([(L - int(rng.integers(800, 9000)), L)] if i % 4 != 2 else []) + \
                 ([(L // 2, L // 2 + 2000)] if i % 5 == 0 else [])
        s = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes())
        for a, b in blocks:
            s[a:b] = tc.telomere(b - a, b"TTAGGG" if a else b"CCCTAA")
        records.append((b"ctg%02d" % i, bytes(s)))
    assert 18_000_000 < sum(len(r[1]) for r in records) < 22_000_000
    fa = tmp_path / "big.fa"
    fa.write_bytes(tc.fasta(records))
    exp = tc.expected(records)
    assert exp["total"] >= 30 and exp["two"] >= 5 and exp["one"] >= 5
    want = hashlib.sha256(tc.bed_text(records, exp)).hexdigest()
    for env in ({}, tc.HOST):
        got = tc.run_cli(cli, ["telostats", str(fa)], str(tmp_path), env)
        assert got["rc"] == 0 and got["out"] == tc.stdout_text(str(fa), exp), got["err"][-1500:]
        assert hashlib.sha256((tmp_path / "big.windows.0.4.50kb.ends.bed").read_bytes()).hexdigest() == want
        os.remove(tmp_path / "big.windows.0.4.50kb.ends.bed")


# ---- the handle's state -------------------------------------------------------------------------------------------------------------------
def many_regions(rng, n=40):
    """one record with n separate telomeric blocks, 5 kb apart, and a quiet record"""
    L = 5000 * n + 3000
    return [(b"many", tc.planted(rng, L, [(5000 * i + 1000, 5000 * i + 2500) for i in range(n)])), (b"quiet", tc.background(rng, 4000))]


def test_two_merge_distances_on_one_handle(acc):
    """no flag, head or tail of the first call is left for the second: each call gives its own result, in either order"""
    records = many_regions(np.random.default_rng(55))
    asm = acc.asm_upload([r[1] for r in records])
    thr = acc.telowin_threshold(0.4, 99.9)
    E = len(records[0][1])
    exps = {d: tc.expected(records, d=d, E=E)["rows"] for d in (100, 5000)}
    assert len(exps[100]) == 40 and len(exps[5000]) == 1
    for d in (100, 5000, 100, 5000, 5000, 100):
        rows = acc.telo_ends(asm, b"TTAGGG", thr, d, E)
        assert [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in rows] == exps[d], d
    asm.close()


def test_more_window_words_than_one_scan_tile(acc):
    """te_order scans the heads and the tails of every word of 64 windows (m = 2, stride 2), four words per window tile, and a tile of the
    scan holds 4096 of them.  A record has one window tile per 256 visited windows and at least one: 2100 records of 0.3 to 2.5 kb and three
    of 2 or 3 window tiles are more than 8192 words, 3 tiles of the scan.  Regions lie in records all along the list, so the places of
    the heads and tails behind the first tile of the scan decide the rows."""
    rng = np.random.default_rng(57)
    records = []
    for i in range(2100):
        L = int(rng.integers(300, 2501))
        n = int(rng.integers(250, 700))
        blocks = [[], [(0, min(L, n))], [(max(0, L - n), L)], [(0, min(L, n)), (max(0, L - n), L)]][i % 4 if i % 5 else 0]
        records.append((b"r%d" % i, tc.planted(rng, L, blocks, b"TTAGGG" if i % 2 else b"CCCTAA")))
    for at, L in ((50, 60000), (1100, 110000), (2099, 52300)):
        records[at] = (b"long%d" % at, tc.planted(rng, L, [(0, 1500), (51000, 51600), (L - 1200, L)]))
    n_words = 4 * sum((tc.visited(len(s)) - 1) // 256 + 1 for _, s in records)      # the tiling rule of ensure_tw_layout, 4 words of 64 windows per tile
    assert n_words > 2 * 4096
    E = 400
    exp = tc.expected(records, E=E)
    assert exp["total"] > 1000 and exp["two"] > 100 and exp["rows"][-1][0] == 2099 and exp["c"][1100] >= 2
    assert device_rows(acc, records, E=E) == exp["rows"]


def test_region_list_sized_too_small(dacc, monkeypatch):
    """the development build takes the size of the region list from CORNETTO_TE_CAP_FORCE: with room for 3 regions the counted total does not
    fit, the placement is rerun with the true size and all rows come back; so they do from the next call, forced small again or not"""
    records = many_regions(np.random.default_rng(56))
    E = 60000
    exp = tc.expected(records, E=E)["rows"]
    assert len(exp) > 6
    asm = dacc.asm_upload([r[1] for r in records])
    thr = dacc.telowin_threshold(0.4, 99.9)
    for force in ("3", "3", None, "1", None):
        if force is None:
            monkeypatch.delenv("CORNETTO_TE_CAP_FORCE", raising=False)
        else:
            monkeypatch.setenv("CORNETTO_TE_CAP_FORCE", force)
        rows = dacc.telo_ends(asm, b"TTAGGG", thr, 100, E)
        assert [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in rows] == exp, force
    asm.close()
