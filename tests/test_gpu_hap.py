"""GPU: the stable radix sort of csrc/sort.hpp on its own (cn_selftest_sort_pairs of the development build, tests/sort_bind.py) against numpy's
stable argsort, and cornetto_hap_fun() / `noboringbits --panel --hap` on the device against the plain-Python restatement of
scripts/create-hapnetto.sh (hap_cases.py) and the CLI's host path.  Everything is integer arithmetic: every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import cornetto_amd
import hap_cases as hc
import sort_bind as sb

pytestmark = pytest.mark.gpu

T = sb.SO_TILE
# the smallest n at which the digit table (256 x tiles) is more than one tile of the scan (4096 counters), and one sort tile more
N_TABLE = (sb.SCAN_TILE // 256) * T + 1
SIZES = [T - 1, T, T + 1, 3 * T + 7, N_TABLE, N_TABLE + T, 300_007]


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def check_sort(dacc, keys, key_bits=64):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    got_k, got_v = sb.sort_pairs(dacc, keys, np.arange(keys.size, dtype=np.uint32), key_bits)
    assert np.array_equal(got_k, keys[order])
    assert np.array_equal(got_v, order.astype(np.uint32))       # payload = original index: equal keys keep their input order


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sort_small(dacc, n):
    rng = np.random.default_rng(n)
    check_sort(dacc, rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64))
    check_sort(dacc, rng.integers(0, 3, size=n, dtype=np.uint64) << np.uint64(17))
    check_sort(dacc, rng.integers(0, 256, size=n, dtype=np.uint64), 8)


@pytest.mark.parametrize("n", SIZES)
def test_sort_key_sets(dacc, n):
    rng = np.random.default_rng(n)
    full = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    assert int(full.max()) >> 63 == 1
    check_sort(dacc, np.full(n, 0x0123456789ABCDEF, dtype=np.uint64))                            # all equal
    check_sort(dacc, np.arange(n, dtype=np.uint64) * np.uint64(0x10001))                         # ascending
    check_sort(dacc, (np.uint64(n) - np.arange(n, dtype=np.uint64)) * np.uint64(0x10001))        # descending
    check_sort(dacc, rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(56))             # only the top byte varies
    check_sort(dacc, (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(24)) | np.uint64(0xAB00000000CD00EF))   # only one middle byte
    check_sort(dacc, full)                                                                       # 64 random bits
    check_sort(dacc, rng.choice(np.array([5, 1 << 40, (1 << 63) + 9], dtype=np.uint64), size=n))  # 3 distinct keys: stability
    for bits in (8, 40, 64):                                                                     # digits at and above key_bits: zero, not touched
        k = full if bits == 64 else full & np.uint64((1 << bits) - 1)
        check_sort(dacc, k, bits)
        if bits < 64:
            top = rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(bits - 8)           # only the top byte of key_bits varies
            check_sort(dacc, top, bits)


def test_sort_twice_on_one_handle(dacc):
    """a large call, a small one, the large one again: the table and the second pair of arrays of the workspace are reused, nothing stale"""
    rng = np.random.default_rng(5)
    big = rng.integers(0, 1 << 40, size=300_007, dtype=np.uint64)
    small = rng.integers(0, 1 << 40, size=1500, dtype=np.uint64)
    for keys in (big, small, big, small[:1], big[:T + 1]):
        check_sort(dacc, keys, 40)


# ---- cornetto_hap_fun ----------------------------------------------------------------------------------------------------------------
def run_hap(acc, lens, haps, D, F):
    got = acc.hap_fun(lens, hc.to_device_rows(haps), merge_dist=D, flank=F)
    return [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in got]


def test_hap_fun_hand_worked(acc, golden_dir):
    names, lens, haps, fun_exp, dip_exp = hc.golden_case(golden_dir)
    got = acc.hap_fun(lens, hc.to_device_rows(haps))                                             # the script's constants are the defaults
    assert [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in got] == fun_exp
    panel = cornetto_amd.panel_boring(lens, got, np.zeros(0, cornetto_amd.IVL_DT))
    assert [tuple(int(x) for x in r) for r in panel] == dip_exp


@pytest.mark.parametrize("seed", range(12))
def test_hap_fun_random(acc, seed):
    lens, haps, D, F = hc.random_case(seed)
    assert run_hap(acc, lens, haps, D, F) == hc.hap_fun(lens, haps, D, F)


def _presorted(haps):
    return [sorted(rows, key=lambda r: (r[1], r[2], r[3], r[0])) for rows in haps]


@pytest.fixture(scope="module")
def planted_small():
    lens, haps, D, F = hc.planted_case(6000, 20, 1, queries_per_hap=60, D=50, max_len=3000, F=20)
    parts = [hc.hap_funbits(lens, rows, D, F) for rows in haps]
    blocks, gaps = sum(len(p[0]) for p in parts), sum(p[2] for p in parts)
    exp = hc.hap_fun(lens, haps, D, F)
    assert blocks > 4096 and gaps > 4096 and len(exp) > 100       # past the merge tile (1024) and the scan tile (4096) in blocks, corners and gaps
    return lens, haps, D, F, exp


@pytest.fixture(scope="module")
def planted_large():
    lens, haps, D, F = hc.planted_case(200_000, 300, 2, queries_per_hap=40)
    return lens, haps, D, F, hc.hap_fun(lens, haps, D, F)


@pytest.mark.parametrize("order", ["shuffled", "presorted"])
def test_hap_fun_planted_small(acc, planted_small, order):
    lens, haps, D, F, exp = planted_small
    assert run_hap(acc, lens, haps if order == "shuffled" else _presorted(haps), D, F) == exp


@pytest.mark.parametrize("order", ["shuffled", "presorted"])
def test_hap_fun_planted_large(acc, planted_large, order):
    lens, haps, D, F, exp = planted_large
    assert len(exp) > 10_000
    assert run_hap(acc, lens, haps if order == "shuffled" else _presorted(haps), D, F) == exp


def test_hap_fun_is_deterministic(acc, planted_large):
    lens, haps, D, F, _exp = planted_large
    rows = hc.to_device_rows(haps)
    a = acc.hap_fun(lens, rows, merge_dist=D, flank=F).tobytes()
    b = acc.hap_fun(lens, rows, merge_dist=D, flank=F).tobytes()
    assert a == b and len(a) > 0


def test_hap_fun_structural_cases(acc):
    D, F = 1000, 500
    lens = [10_000, 4000, 0, 700]
    cases = {
        "one row": [[(b"q", 0, 600, 900)]],
        "one group": [[(b"q", 0, s, s + 300) for s in range(0, 9000, 700)]],                     # gaps of 400 <= D: one block
        "every row its own query": [[(b"q%d" % i, 0, s, s + 300) for i, s in enumerate(range(0, 9000, 700))]],
        "a contig covered exactly": [[(b"q", 1, 0, 4000), (b"r", 3, 0, 700)]],                   # no gap there, right corners beyond the end
        "n_rows = [0, k]": [[], [(b"q", 0, 0, 10_000), (b"q", 1, 100, 200)]],
        "no rows at all": [[], []],
        "gap of exactly D and of D + 1": [[(b"q", 0, 0, 100), (b"q", 0, 1100, 1200), (b"q", 0, 2201, 2300)]],
    }
    for name, haps in cases.items():
        exp = hc.hap_fun(lens, haps, D, F)
        assert run_hap(acc, lens, haps, D, F) == exp, name
    # spelled out: the covered contig has no gap and its right corner is not clamped
    got = run_hap(acc, lens, cases["a contig covered exactly"], D, F)
    assert (1, 3500, 4500) in got and (3, 200, 1200) in got and not any(r[0] == 1 and r[1] == 0 for r in got)
    assert run_hap(acc, lens, cases["no rows at all"], D, F) == [(0, 0, 10_000), (1, 0, 4000), (3, 0, 700)]
    assert run_hap(acc, lens, [], D, F) == []                                                    # no haplotype: nothing is fun
    assert run_hap(acc, [], [[]], D, F) == []


def test_hap_fun_rejects_bad_rows(acc):
    lens = [1000, 2000]
    for row in [(0, 2, 0, 10), (0, -1, 0, 10), (0, 0, 10, 10), (0, 0, 20, 10), (0, 0, -1, 10)]:
        with pytest.raises(cornetto_amd.AccelError) as e:
            acc.hap_fun(lens, [np.array([(0, 0, 5, 9), row], cornetto_amd.HAP_ROW_DT)])
        assert e.value.status == -3                                                              # CORNETTO_E_ARG
    with pytest.raises(cornetto_amd.AccelError):
        acc.hap_fun(lens, [np.array([(0, 0, 5, 9)], cornetto_amd.HAP_ROW_DT)], flank=0)


def test_hap_fun_is_timed(acc, golden_dir):
    names, lens, haps, fun_exp, _ = hc.golden_case(golden_dir)
    acc.hap_fun(lens, hc.to_device_rows(haps))
    C = cornetto_amd.C
    n = acc.L.cornetto_accel_last_timing(acc.h, None, None, 0)
    nm, ms = (C.c_char_p * n)(), (C.c_float * n)()
    acc.L.cornetto_accel_last_timing(acc.h, nm, ms, n)
    seen = set(x.decode() for x in nm)
    assert {"hp_sort_pos", "hp_sort_query", "hp_block_merge", "hp_corners", "hp_gap_write", "hp_fun_merge"} <= seen, seen
    assert all(m >= 0 for m in ms)


# ---- the CLI on the device against its host path ---------------------------------------------------------------------------------------
def test_cli_device_equals_host_path(golden_dir, tmp_path):
    from helpers import read_bedgraph_pair
    tot, mq = tmp_path / "tot.bg", tmp_path / "mq.bg"
    tot.write_bytes(gzip.open(os.path.join(golden_dir, "cov-total.bg.gz")).read())
    mq.write_bytes(gzip.open(os.path.join(golden_dir, "cov-mq20.bg.gz")).read())
    trip = read_bedgraph_pair(str(tot), str(mq))
    names, lens = [t[0] for t in trip][::-1] + [b"only_in_assembly"], [len(t[1]) for t in trip][::-1] + [5000]
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, l) for n, l in zip(names, lens)))
    _l, haps, D, F = hc.random_case(4, lens=list(lens), max_queries=12, DF=(1500, 40))
    haps = (haps + haps)[:2]
    opts = ["-w", "1000", "-i", "100", "-e", "2000", "-m", "10000", "--panel", str(tmp_path / "asm.bed"), "--panel-params", "300,2000,500,700,3000,2500,4000",
            "--hap-params", "%d,%d" % (D, F)]
    for k, rows in enumerate(haps):
        (tmp_path / ("hap%d.paf" % k)).write_bytes(hc.paf_text(names, lens, rows[k:]))
        opts += ["--hap", str(tmp_path / ("hap%d.paf" % k))]
    res = {}
    for mode in ("dev", "host"):
        args = [cornetto_amd.CLI_PATH, "noboringbits"] + (["--accel=no"] if mode == "host" else []) + [str(tot), "-q", str(mq)] + opts
        args += ["--dip", str(tmp_path / (mode + ".dip.bed")), "--hap-fun", str(tmp_path / (mode + ".fun.bed"))]
        p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res[mode] = (p.stdout, (tmp_path / (mode + ".dip.bed")).read_bytes(), (tmp_path / (mode + ".fun.bed")).read_bytes())
        p = subprocess.run(args[:-4], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)        # --hap alone: stdout is the diploid panel
        assert p.returncode == 0 and p.stdout == res[mode][1], p.stderr.decode()[-2000:]
    assert res["dev"] == res["host"]
    assert res["dev"][0] and res["dev"][1] and res["dev"][0] != res["dev"][1]
    assert res["dev"][2] == hc.bed_text(names, hc.hap_fun(lens, [haps[0], haps[1][1:]], D, F))
