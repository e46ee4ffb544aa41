"""CPU: `cornetto telostats` on the host path (CORNETTO_ACCEL=no, no visible GPU) and its AddressSanitizer build against the restatement of
scripts/telostats.sh in tests/telostats_cases.py (oracle telofind / telowin + a sequential merge + the ends rule): the BED, stdout, the name
of the default BED, usage and exit codes, rejected options; the run-length rule the device stage merges by (csrc/telostats.hip), modelled
word by word, against the sequential `bedtools merge`; and `cornetto telocontigs` on the BED that telostats wrote."""
import os

import numpy as np
import pytest

import cornetto_amd
import telostats_cases as tc
from helpers import build_asan_cli, read_fastx

HOST = tc.HOST
DS = [0, 1, 99, 100, 199, 200, 201, 999, 1000, 5000, 11799]
LS = [0, 1, 199, 200, 999, 1000, 1001, 1200, 1201]


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


@pytest.fixture(scope="module")
def asan_cli():
    return build_asan_cli()


@pytest.mark.parametrize("d", DS)
def test_the_run_rule_is_the_sequential_merge(d):
    """head = q[j] with no q in [j - G, j - 1], tail = q[j] with no q in [j + 1, j + G], G = (1000 + d) / 200, r-th head with r-th tail ==
    bedtools merge -d d over the qualifying windows in start order: every length at which the window loop changes, random lengths up to
    30 000, sparse, dense and clustered qualification bits"""
    rng = np.random.default_rng(1000 + d)
    lens = LS + [int(x) for x in rng.integers(0, 30001, size=120)] + [25600 + 1000, 51200 + 800, 51201 + 1000]
    n = 0
    for L in lens:
        J = tc.visited(L)
        for p in (0.0, 0.02, 0.1, 0.3, 0.7, 1.0):
            q = rng.random(J) < p
            if p == 0.3 and J > 8:           # clusters with gaps around G
                q[:] = False
                j = 0
                while j < J:
                    run = int(rng.integers(1, 6))
                    q[j:j + run] = True
                    j += run + int(rng.integers(1, (1000 + d) // 200 + 4))
            wins = [tc.window_of(j, L) for j in range(J) if q[j] and tc.window_of(j, L)[1] > tc.window_of(j, L)[0]]
            qq = [bool(q[j]) and tc.window_of(j, L)[1] > tc.window_of(j, L)[0] for j in range(J)]
            assert tc.run_rule(qq, L, d) == tc.merge(wins, d), (L, d, p)
            n += 1
    assert n >= 700


def small_assemblies():
    rng = np.random.default_rng(77)
    return [tc.random_assembly(rng, 40_000) for _ in range(12)]


@pytest.mark.parametrize("k", range(12))
def test_small_assembly_host_and_asan(cli, asan_cli, tmp_path, k):
    recs = small_assemblies()[k]
    rng = np.random.default_rng(500 + k)
    d = int(rng.choice(DS))
    E = int(rng.choice([1, 200, 999, 5000, 20000, 50000]))
    t = str(rng.choice(["0.4", "0.1", "0.05", "0.9", "1"]))
    fa = tmp_path / "asm.fa"
    fa.write_bytes(tc.fasta(recs, int(rng.choice([60, 61, 1000]))))
    exp = tc.expected(recs, b"TTAGGG", float(t), 99.9, d, E)
    opts = ["-t", t, "-d", str(d), "-e", str(E)]
    a = tc.check_cli(cli, recs, str(fa), str(tmp_path), HOST, opts, t=t, d=d, E=E, exp=exp)
    b = tc.check_cli(asan_cli, recs, str(fa), str(tmp_path), HOST, opts, t=t, d=d, E=E, exp=exp)
    assert a == b


def test_some_small_assembly_has_rows():
    exps = [tc.expected(r, d=100, E=5000) for r in small_assemblies()]
    assert sum(e["total"] for e in exps) >= 10 and any(e["two"] for e in exps) and any(e["one"] for e in exps)


@pytest.mark.parametrize("name,opts,kw", [
    ("mix.fa.gz", [], {}),
    ("mix.fa.gz", ["-e", "300", "-t", "0.1"], {"E": 300, "t": "0.1"}),
    ("mix.fa.gz", ["-m", "TTAGGGTTAGGG", "-e", "2000", "-i", "95"], {"m": b"TTAGGGTTAGGG", "E": 2000, "I": "95"}),
    ("probe.fa", [], {}),
    ("probe.fa", ["-e", "1000", "-d", "0"], {"E": 1000, "d": 0}),
    ("probe_selfoverlap.fa", ["-m", "ACACA", "-t", "0.01", "-e", "10"], {"m": b"ACACA", "t": "0.01", "E": 10}),
])
def test_golden_inputs(cli, asan_cli, golden_dir, tmp_path, name, opts, kw):
    path = os.path.join(golden_dir, name)
    recs = [(r[0], r[2]) for r in read_fastx(path)]
    a = tc.check_cli(cli, recs, path, str(tmp_path), HOST, opts, **kw)
    b = tc.check_cli(asan_cli, recs, path, str(tmp_path), HOST, opts, **kw)
    assert a == b


def test_the_golden_inputs_have_regions(golden_dir):
    recs = [(r[0], r[2]) for r in read_fastx(os.path.join(golden_dir, "mix.fa.gz"))]
    assert tc.expected(recs, E=300, t=0.1)["total"] > 0


@pytest.mark.parametrize("fname,bed", [("x.fa", "x.windows.0.4.50kb.ends.bed"), ("x.fasta", "x.windows.0.4.50kb.ends.bed"),
                                       ("x.fa.gz", "x.fa.gz.windows.0.4.50kb.ends.bed"), ("sub/y.v2.fasta", "y.v2.windows.0.4.50kb.ends.bed")])
def test_default_bed_name(cli, tmp_path, fname, bed):
    import gzip
    rng = np.random.default_rng(3)
    recs = [(b"a", tc.planted(rng, 5000, [(0, 1500)])), (b"b", tc.background(rng, 700))]
    text = tc.fasta(recs)
    os.makedirs(tmp_path / "sub", exist_ok=True)
    (tmp_path / fname).write_bytes(gzip.compress(text, 6, mtime=0) if fname.endswith(".gz") else text)
    assert tc.default_bed_name(fname) == bed
    got = tc.run_cli(cli, ["telostats", fname], str(tmp_path), HOST)
    exp = tc.expected(recs)
    assert got["rc"] == 0 and got["out"] == tc.stdout_text(fname, exp), got["err"][-1500:]
    assert exp["total"] == 1 and (tmp_path / bed).read_bytes() == tc.bed_text(recs, exp)
    # -t as typed and -e in kb (%.0f) in the name; -b overrides it
    got = tc.run_cli(cli, ["telostats", "-t", "0.40", "-e", "2500", fname], str(tmp_path), HOST)
    assert got["rc"] == 0 and os.path.exists(tmp_path / tc.default_bed_name(fname, "0.40", 2500)), got["err"][-1500:]
    assert tc.default_bed_name(fname, "0.40", 2500).endswith(".windows.0.40.2kb.ends.bed")
    before = sorted(os.listdir(tmp_path))
    got = tc.run_cli(cli, ["telostats", "-b", "other.bed", fname], str(tmp_path), HOST)
    assert got["rc"] == 0 and sorted(os.listdir(tmp_path)) == sorted(before + ["other.bed"])
    assert (tmp_path / "other.bed").read_bytes() == tc.bed_text(recs, exp)


def test_usage_and_exit_codes(cli, tmp_path):
    rng = np.random.default_rng(4)
    (tmp_path / "a.fa").write_bytes(tc.fasta([(b"a", tc.planted(rng, 3000, [(0, 1200)]))]))
    got = tc.run_cli(cli, ["telostats"], str(tmp_path), HOST)
    assert got["rc"] == 1 and got["out"] == b"" and b"Usage: cornetto telostats" in got["err"] and b"not pooled" in got["err"]
    got = tc.run_cli(cli, ["telostats", "-h"], str(tmp_path), HOST)
    assert got["rc"] == 0 and b"Usage: cornetto telostats" in got["out"] and b"not pooled" in got["out"]
    got = tc.run_cli(cli, ["telostats", "a.fa", "b.fa"], str(tmp_path), HOST)
    assert got["rc"] == 1 and got["out"] == b""
    got = tc.run_cli(cli, ["telostats", "nonexistent.fa"], str(tmp_path), HOST)
    assert got["rc"] == 1 and got["out"] == b"" and b"Could not to open file nonexistent.fa" in got["err"]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".bed")]
    for bad in (["-d", "11800"], ["-d", "-1"], ["-d", "x"], ["-t", "0"], ["-t", "-0.4"], ["-t", "nan"], ["-e", "0"], ["-m", ""]):
        got = tc.run_cli(cli, ["telostats"] + bad + ["a.fa"], str(tmp_path), HOST)
        assert got["rc"] == 1 and got["out"] == b"", (bad, got["out"])
        assert not [f for f in os.listdir(tmp_path) if f.endswith(".bed")], bad
    got = tc.run_cli(cli, ["telostats", "-d", "11799", "a.fa"], str(tmp_path), HOST)
    assert got["rc"] == 0 and b"Merge telomere motifs in 11799bp\n" in got["out"]
    # the 3-line footer of every sub-command and telowin's line on stderr
    assert b"Given error rate of 0.999000 running with adjusted threshold of 0.397606" in got["err"] and b"] CMD: " in got["err"] and b"Real time" in got["err"]
    got = tc.run_cli(cli, ["--help"], str(tmp_path), HOST)
    assert b"telostats" in got["out"]


def test_telocontigs_reads_the_bed(cli, tmp_path):
    """`cornetto telocontigs asm.fa <the BED telostats wrote>` prints, per contig, the c of expected()"""
    rng = np.random.default_rng(5)
    E = 4000
    recs = [(b"both", tc.planted(rng, 20000, [(0, 2500), (18000, 20000)])), (b"none", tc.background(rng, 9000)),
            (b"left", tc.planted(rng, 12345, [(0, 1800)])), (b"whole", tc.telomere(2 * E + 200)), (b"inner", tc.planted(rng, 30000, [(14000, 16000)])),
            (b"short", tc.telomere(700)), (b"three", tc.planted(rng, 26000, [(0, 1200), (2700, 3900), (24000, 26000)]))]
    (tmp_path / "asm.fa").write_bytes(tc.fasta(recs))
    exp = tc.expected(recs, E=E)
    assert exp["c"] == [2, 0, 1, 2, 0, 1, 3] and (exp["one"], exp["two"], exp["more"]) == (2, 2, 1)
    tc.check_cli(cli, recs, "asm.fa", str(tmp_path), HOST, ["-e", str(E)], E=E, exp=exp)
    got = tc.run_cli(cli, ["telocontigs", "asm.fa", "out.bed"], str(tmp_path), HOST)
    assert got["rc"] == 0, got["err"][-1500:]
    order = sorted(range(len(recs)), key=lambda i: -len(recs[i][1]))
    assert got["out"] == b"Contig\tLength\tNTelomeres\n" + b"".join(b"%s\t%d\t%d\n" % (recs[i][0], len(recs[i][1]), exp["c"][i]) for i in order)


@pytest.mark.parametrize("name,d", [("merge_default", 0), ("merge_d1000", 1000)])
def test_the_restatement_merges_as_the_bedtools_manual(golden_dir, name, d):
    """the sweep of telostats_cases.merge() on the worked examples of the bedtools manual (tests/golden/bedtools/README.md)"""
    def rows(f):
        return [(t[0], int(t[1]), int(t[2])) for t in (ln.split() for ln in open(os.path.join(golden_dir, "bedtools", f))) if len(t) >= 3]
    got = []
    inp = rows(name + ".in.bed")
    for c in sorted(set(r[0] for r in inp), key=[r[0] for r in inp].index):
        got += [(c, s, e) for s, e in tc.merge(sorted((s, e) for cc, s, e in inp if cc == c), d)]
    assert got == rows(name + ".exp.bed")
