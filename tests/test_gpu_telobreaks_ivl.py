"""GPU: the telomere breaks by the rule on intervals (csrc/telobreaks_ivl.hip) — cornetto_telobreaks_ivl() on explicit lists, cornetto_telo_breaks()
on resident assemblies and `cornetto telostats --breaks` on the device path — against the rule restated in tests/telobreaks_cases.py, the
bitset kernels of cornetto_telobreaks() and the oracle chain (sdust + telofind + the reference's two bitsets).  The planted lists put a row
where bk_mark decides: the flank on and one base off either edge of an interval, both clips, an interval beyond the contig's end, the
24-base limit, a row whose binary search lands in the previous contig or in front of the list, more intervals than three tiles of the scan;
every one asserts on the expected data that it has the property it is named after."""
import hashlib
import os

import numpy as np
import pytest

import cornetto_amd
import oracle_bind as ob
import telobreaks_cases as bc
import telostats_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def triples(rows):
    return [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in rows]


def device_ivl(acc, lens, sd, tel, fn="telobreaks_ivl"):
    sd = np.array(sd, dtype=cornetto_amd.IVL_DT) if sd else np.zeros(0, cornetto_amd.IVL_DT)
    tel = np.array(tel, dtype=cornetto_amd.TELROW_DT) if tel else np.zeros(0, cornetto_amd.TELROW_DT)
    return triples(getattr(acc, fn)(np.array(lens, np.int32), sd, tel))


def device_breaks(acc, records, m=b"TTAGGG", T=20, W=64):
    asm = acc.asm_upload([r[1] for r in records])
    try:
        return triples(acc.telo_breaks(asm, m, T, W))
    finally:
        asm.close()


# ---- planted explicit lists: name -> (lens, sd, tel, property of the case and of the expected rows) --------------------------------------
def flanks(lens, row):
    c, s, e, _ = row
    return max(0, s - 100), min(lens[c], e + 100)


def planted_lists():
    cases = {}
    row = (0, 300, 340, 40)

    def prop_exact(lens, sd, tel, exp):
        assert flanks(lens, tel[0]) == (sd[0][1], sd[0][2]) and exp == [(0, 199, 439)]
    cases["flank_equals_the_interval"] = ([1000], [(0, 200, 440)], [row], prop_exact)

    def prop_left(lens, sd, tel, exp):
        a, b = flanks(lens, tel[0])
        assert sd[0][1] == a + 1 and sd[0][2] == b and exp == []
    cases["flank_one_base_short_on_the_left"] = ([1000], [(0, 201, 440)], [row], prop_left)

    def prop_right(lens, sd, tel, exp):
        a, b = flanks(lens, tel[0])
        assert sd[0][1] == a and sd[0][2] == b - 1 and exp == []
    cases["flank_one_base_short_on_the_right"] = ([1000], [(0, 200, 439)], [row], prop_right)

    def prop_clip0(lens, sd, tel, exp):
        assert tel[0][1] - 100 < 0 and flanks(lens, tel[0]) == (0, 190) and exp == [(0, 0, 189)]
    cases["a_clipped_at_0"] = ([1000], [(0, 0, 190)], [(0, 50, 90, 40)], prop_clip0)

    def prop_clipL(lens, sd, tel, exp):
        assert tel[0][2] + 100 > lens[0] and flanks(lens, tel[0]) == (800, 1000) and exp == [(0, 799, 999)]
    cases["b_clipped_at_L"] = ([1000], [(0, 800, 1000)], [(0, 900, 960, 60)], prop_clipL)

    def prop_past(lens, sd, tel, exp):
        assert sd[0][2] > lens[0] and tel[0][2] == lens[0] and exp == [(0, 799, 999)]
    cases["interval_beyond_the_contig_end"] = ([1000], [(0, 800, 1040)], [(0, 950, 1000, 50)], prop_past)

    def prop_24(lens, sd, tel, exp):
        assert [t[3] for t in tel] == [23, 24] and exp == [(0, 499, 799)]
    cases["matched_23_next_to_24"] = ([1000], [(0, 100, 400), (0, 500, 800)], [(0, 200, 223, 23), (0, 600, 624, 24)], prop_24)

    def prop_neighbour(lens, sd, tel, exp):
        a, _ = flanks(lens, tel[0])
        assert all(v[0] != tel[0][0] for v in sd) and sd[-1][0] == tel[0][0] - 1 and sd[-1][1] <= a and sd[-1][2] >= tel[0][2] + 100 and exp == []
    cases["row_in_a_contig_without_intervals"] = ([1000, 1000], [(0, 100, 900)], [(1, 300, 340, 40)], prop_neighbour)

    def prop_front(lens, sd, tel, exp):
        assert flanks(lens, tel[0])[0] < sd[0][1] and sd[0][0] == 0 and exp == []
    cases["row_before_the_first_interval"] = ([1000], [(0, 500, 900)], [(0, 100, 140, 40)], prop_front)

    def prop_two(lens, sd, tel, exp):
        assert len(tel) == 2 and exp == [(0, 99, 899)]
    cases["two_rows_in_one_interval"] = ([1000], [(0, 100, 900)], [(0, 300, 340, 40), (0, 500, 540, 40)], prop_two)

    def prop_len0(lens, sd, tel, exp):
        assert lens[0] == 0 and lens[2] == 0 and exp == [(1, 99, 899)]
    cases["contig_of_length_0"] = ([0, 1000, 0], [(0, 0, 30), (1, 100, 900)], [(1, 300, 340, 40)], prop_len0)

    def prop_empty(lens, sd, tel, exp):
        assert (not sd or not tel) and exp == []
    cases["empty_sd"] = ([1000], [], [row], prop_empty)
    cases["empty_tel"] = ([1000], [(0, 200, 440)], [], prop_empty)
    cases["empty_sd_and_tel"] = ([1000], [], [], prop_empty)
    cases["no_contig"] = ([], [], [], prop_empty)

    # 13 000 intervals over three contigs, a row in every third one: the ranks of the marked intervals cross three tile seams of the scan
    lens, sd, tel = [], [], []
    for c, k in enumerate((4400, 4400, 4200)):
        lens.append(400 * k)
        sd += [(c, 400 * i, 400 * i + 300) for i in range(k)]
        tel += [(c, 400 * i + 120, 400 * i + 160, 40) for i in range(c, k, 3)]

    def prop_many(lens, sd, tel, exp):
        assert len(sd) > 3 * 4096 and len(exp) == len(tel) > 4096 and exp[0][:2] == (0, 0) and exp[-1][0] == 2 and exp[-1][2] >= lens[2] - 1000
        idx = [sd.index((c, s + 1 if s else 0, e + 1)) for c, s, e in exp[::400] + exp[-1:]]
        assert min(idx) < 4096 and max(idx) > 3 * 4096
    cases["more_intervals_than_three_scan_tiles"] = (lens, sd, tel, prop_many)
    return cases


LISTS = planted_lists()


@pytest.mark.parametrize("name", sorted(LISTS))
def test_planted_lists(acc, name):
    lens, sd, tel, prop = LISTS[name]
    exp = bc.rule(lens, sd, tel)
    prop(lens, sd, tel, exp)
    assert bc.oracle_bitset(lens, sd, tel) == exp
    assert device_ivl(acc, lens, sd, tel, "telobreaks") == exp
    assert device_ivl(acc, lens, sd, tel) == exp


@pytest.mark.parametrize("sd,tel,status", [
    ([(0, 500, 800), (0, 100, 400)], [(0, 600, 640, 40)], -3),                   # not in start order
    ([(1, 100, 400), (0, 500, 800)], [(0, 600, 640, 40)], -3),                   # not in contig order
    ([(0, 100, 400), (0, 400, 800)], [(0, 600, 640, 40)], -3),                   # touching
    ([(0, 100, 400), (0, 399, 800)], [], -3),                                    # overlapping, and no row
    ([(0, 100, 400), (2, 500, 800)], [(0, 200, 240, 40)], -3),                   # a contig that is not in the table
    ([(0, 100, 400)], [(0, 980, 1001, 40)], -6),                                 # a row beyond the end of its contig
    ([(0, 100, 400)], [(0, -1, 40, 41)], -6),
    ([(0, 100, 400)], [(0, 300, 300, 40)], -6),                                  # start >= end
    ([(0, -5, 400)], [(0, 200, 240, 40)], -6),                                   # an interval with a negative start
])
def test_bad_lists(acc, sd, tel, status):
    with pytest.raises(cornetto_amd.AccelError) as e:
        device_ivl(acc, [1000, 1000], sd, tel)
    assert e.value.status == status
    # the handle is as good as before
    assert device_ivl(acc, [1000], [(0, 200, 440)], [(0, 300, 340, 40)]) == [(0, 199, 439)]


def test_random_soups(acc):
    rng = np.random.default_rng(70)
    n = 0
    for it in range(100):
        lens, sd, tel = bc.random_soup(rng)
        assert bc.precondition(sd)
        exp = bc.oracle_bitset(lens, sd, tel)
        assert bc.rule(lens, sd, tel) == exp, it
        assert device_ivl(acc, lens, sd, tel) == exp, (it, lens, sd, tel)
        n += len(exp)
    print("breaks %d" % n)
    assert n > 50


# ---- resident assemblies -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(10))
def test_random_small_assemblies(acc, part):
    """150 assemblies of 1-6 records of 0-130 kb against the oracle chain; windows of 70 and 100 take the sdust kernel with byte counters
    (W - 2 > 64) instead of the default family.  (The family beyond 257: test_sdust_window_of_258, on short records — the oracle's sdust needs
    minutes per assembly of this size there.)"""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(700 + part)
    cases = []
    for it in range(15):
        records = bc.random_assembly(rng)
        W = int(rng.choice([64, 64, 64, 64, 32, 20, 70, 100 if sum(len(r[1]) for r in records) < 150_000 else 70]))
        cases.append((records, int(rng.choice([20, 20, 10, 30])), W))
    with ThreadPoolExecutor(8) as ex:                  # (the oracle's sdust is most of this test's time, and its calls release the interpreter lock)
        exps = list(ex.map(lambda c: bc.chain_rows(c[0], b"TTAGGG", c[1], c[2]), cases))
    n = 0
    for it, ((records, T, W), exp) in enumerate(zip(cases, exps)):
        assert device_breaks(acc, records, b"TTAGGG", T, W) == exp, (part, it, T, W)
        n += len(exp)
    print("breaks %d" % n)
    assert n > 15


def test_bordered_and_long_motifs(acc):
    rng = np.random.default_rng(71)
    recs = [(b"ac", bc.planted_thin(rng, 40000, [(0, 3000), (20000, 22000), (38000, 40000)], b"ACACA", 170)), (b"quiet", tc.background(rng, 5000)),
            (b"tel", bc.planted_thin(rng, 30000, [(0, 2500), (27000, 30000)], b"TTAGGG", 170))]
    m = b"ACACA"
    assert any(m[:b] == m[-b:] for b in range(1, len(m)))                         # a border: the runs are collected on the host and uploaded
    for motif, ctg in ((m, 0), (b"TTAGGG" * 2, 2)):
        exp = bc.chain_rows(recs, motif)
        assert len(exp) >= 2 and {r[0] for r in exp} == {ctg}, (motif, exp)
        assert device_breaks(acc, recs, motif) == exp, motif


def revcomp(m):
    return bytes({65: 84, 84: 65, 67: 71, 71: 67}[c] for c in m[::-1])


def test_unbordered_motif_of_12(acc):
    """TTAGGGTTAGGC and its reverse complement overlap no copy of themselves: the 16-position automaton of tf_scan, the runs paired and kept
    on the device (TTAGGGTTAGGG above has the border TTAGGG and goes through the host)"""
    m = b"TTAGGGTTAGGC"
    assert not any(x[:b] == x[-b:] for x in (m, revcomp(m)) for b in range(1, len(m))) and 8 < len(m) <= 16
    rng = np.random.default_rng(73)
    recs = [(b"u12", bc.planted_thin(rng, 30000, [(0, 3000), (14000, 16000), (27500, 30000)], m, 170)), (b"quiet", tc.background(rng, 4000)),
            (b"rc", bc.planted_thin(rng, 20000, [(17000, 20000)], revcomp(m), 170))]
    exp = bc.chain_rows(recs, m)
    assert len(exp) == 4 and [r[0] for r in exp] == [0, 0, 0, 2], exp
    assert device_breaks(acc, recs, m) == exp


def test_sdust_window_of_258(acc):
    """W - 2 > 255: the sdust family with its state in global memory leaves its list on the device as the other two do.  (Short records: the
    oracle's sdust takes about a second per 400 low-complexity bases at this window.)"""
    rng = np.random.default_rng(74)
    recs = [(b"w", bc.planted_thin(rng, 1500, [(0, 400)], b"TTAGGG", 120)), (b"e", b""), (b"x", bc.planted_thin(rng, 1300, [(900, 1300)], b"CCCTAA", 90))]
    exp = bc.chain_rows(recs, b"TTAGGG", 20, 258)
    assert len(exp) == 2 and exp != bc.chain_rows(recs), exp
    assert device_breaks(acc, recs, b"TTAGGG", 20, 258) == exp


def test_two_parameter_sets_on_one_handle(acc):
    """nothing of one call's lists, flags or counts is left for the next: each call gives its own result, in either order"""
    records = bc.cli_records()[:1] + [(b"dense", bc.planted_thin(np.random.default_rng(62), 9000, [(3000, 6000)], every=30))]
    exps = {(T, W): bc.chain_rows(records, b"TTAGGG", T, W) for T, W in ((20, 64), (40, 64))}
    assert len(exps[20, 64]) == 3 and len(exps[40, 64]) == 2
    asm = acc.asm_upload([r[1] for r in records])
    for T, W in ((20, 64), (40, 64), (20, 64), (40, 64), (40, 64), (20, 64)):
        assert triples(acc.telo_breaks(asm, b"TTAGGG", T, W)) == exps[T, W], (T, W)
    asm.close()


def test_assembly_of_20_mbases(acc, cli, tmp_path):
    """30 contigs with thinned telomere blocks at some ends and in the middle: cornetto_telo_breaks(), the CLI on the device path, the CLI on
    the host path and the oracle chain agree (sha256 of the rows / of the file)"""
    rng = np.random.default_rng(72)
    records = []
    for i in range(30):
        L = int(rng.integers(300_000, 1_050_000))
        blocks = ([(0, int(rng.integers(800, 9000)))] if i % 3 != 1 else []) + ([(L - int(rng.integers(800, 9000)), L)] if i % 4 != 2 else []) + \
                 ([(L // 2, L // 2 + 2000)] if i % 5 == 0 else [])
        s = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes())
        for a, b in blocks:
            s[a:b] = bc.thinned_telomere(b - a, int(rng.integers(60, 400)), b"TTAGGG" if a else b"CCCTAA")
        records.append((b"ctg%02d" % i, bytes(s)))
    assert 18_000_000 < sum(len(r[1]) for r in records) < 22_000_000
    exp = bc.chain_rows_threaded(records)
    assert len(exp) >= 30 and len({r[0] for r in exp}) >= 20
    want_rows = hashlib.sha256(np.array(exp, dtype=cornetto_amd.IVL_DT).tobytes()).hexdigest()
    asm = acc.asm_upload([r[1] for r in records])
    got = acc.telo_breaks(asm)
    asm.close()
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want_rows
    fa = tmp_path / "big.fa"
    fa.write_bytes(tc.fasta(records))
    want = hashlib.sha256(bc.breaks_text(records, exp)).hexdigest()
    for env in ({}, bc.HOST):
        got = bc.run_breaks(cli, str(fa), str(tmp_path), env)
        assert got["rc"] == 0, got["err"][-1500:]
        assert hashlib.sha256(got["breaks"]).hexdigest() == want, env


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("telobreaks_cli")
    records = bc.cli_records()
    bc.write_inputs(d, records)
    want = bc.expected_text(records)
    host = {}
    for f in ("asm.fa", "asm.fq"):
        hd = tmp_path_factory.mktemp("host")
        got = bc.run_breaks(cli, str(d / f), str(hd), bc.HOST, ["-e", "2000"])
        assert got["rc"] == 0 and got["breaks"] == want, got["err"][-1500:]
        host[f] = (got["out"], got["bed"], got["breaks"])
    return d, host


@pytest.mark.parametrize("fname", ["asm.fa", "asm.fq"])
@pytest.mark.parametrize("env", [{}, {"CORNETTO_CLI_WHOLE": "0"}, {"CORNETTO_FASTQ_PIECE": "4096"}, {"CORNETTO_BATCH_BASES": "30000"},
                                 {"CORNETTO_BATCH_BASES": "30000", "CORNETTO_FASTQ_SPLIT": "host"}, {"CORNETTO_DEVICES": "0,0"}],
                         ids=["whole", "pieces", "small_pieces", "small_batches", "sequential_small_batches", "first_listed_device"])
def test_cli_routes(cli, cli_case, tmp_path, env, fname):
    d, host = cli_case
    got = bc.run_breaks(cli, str(d / fname), str(tmp_path), env, ["-e", "2000"])
    assert got["rc"] == 0, got["err"][-1500:]
    assert (got["out"], got["bed"], got["breaks"]) == host[fname]


def test_records_that_share_a_name(cli, tmp_path):
    records, want = bc.shared_name_case()
    bc.write_inputs(tmp_path, records)
    for env in ({}, {"CORNETTO_BATCH_BASES": "30000"}):
        got = bc.run_breaks(cli, str(tmp_path / "asm.fa"), str(tmp_path), env)
        assert got["rc"] == 0 and got["breaks"] == want, (env, got["err"][-1500:])


def test_the_device_path_is_taken(cli, cli_case, tmp_path):
    """CORNETTO_DEVICE names a device that does not exist: exit 1 and no line in the breaks file (no silent host fallback)"""
    d, host = cli_case
    got = bc.run_breaks(cli, str(d / "asm.fa"), str(tmp_path), {"CORNETTO_DEVICE": "999"}, ["-e", "2000"])
    assert got["rc"] == 1 and b"cannot open HIP device" in got["err"] and b"total telomere regions" not in got["out"]
    assert not got["breaks"]


def test_kernels_of_the_call(acc):
    """the call runs sdust, the telomere scan and the three interval kernels, and none of the bitset kernels"""
    asm = acc.asm_upload([r[1] for r in bc.cli_records()])
    acc.telo_breaks(asm)
    names = {n for n, _ in acc.last_timing()}
    asm.close()
    assert {"bk_check", "bk_mark", "bk_scan", "bk_emit", "tf_scan"} <= names and not any(n.startswith("tb_") for n in names), names
    assert any(n.startswith("sd") for n in names), names
