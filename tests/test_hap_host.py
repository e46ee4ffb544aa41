"""CPU (no GPU anywhere): `noboringbits --panel ... --hap FILE` on the host path (--accel=no: cli/host_backend.c cli_host_hap_fun, the PAF reader
of cli/tables.c), the plain build and the AddressSanitizer + UBSan build, against the plain-Python restatement of scripts/create-hapnetto.sh
in hap_cases.py and the hand-worked case of tests/golden/hapnetto.  PARITY UNPINNED (no bedtools); every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import cornetto_amd
import oracle_bind as ob
import hap_cases as hc

NO_GPU = {"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}
COV_OPTS = ["-w", "1000", "-i", "100", "-e", "2000", "-m", "10000"]
PANEL_PAR = (300, 2000, 500, 700, 3000, 2500, 4000)          # test_panel.py::test_noboringbits_panel_mode_cli: the small contigs qualify


@pytest.fixture(scope="module", params=["product", "asan"])
def cli(request):
    if request.param == "product":
        assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
        return cornetto_amd.CLI_PATH
    from helpers import build_asan_cli
    return build_asan_cli()


@pytest.fixture(scope="module")
def product():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def run(cli, args):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", LSAN_OPTIONS="exitcode=0", UBSAN_OPTIONS="print_stacktrace=1")
    e.pop("CORNETTO_ACCEL", None)
    e.update(NO_GPU)
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
    assert p.returncode != 99 and b"runtime error" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def cov(golden_dir, tmp_path_factory):
    """the committed coverage pair, uncompressed: (total, mq20, contig names, contig lengths)"""
    from helpers import read_bedgraph_pair
    d = tmp_path_factory.mktemp("hap_host")
    tot, mq = d / "tot.bg", d / "mq.bg"
    tot.write_bytes(gzip.open(os.path.join(golden_dir, "cov-total.bg.gz")).read())
    mq.write_bytes(gzip.open(os.path.join(golden_dir, "cov-mq20.bg.gz")).read())
    trip = read_bedgraph_pair(str(tot), str(mq))
    return str(tot), str(mq), [t[0] for t in trip], [len(t[1]) for t in trip]


def base_args(cov, asm_bed):
    return ["noboringbits", "--accel=no", cov[0], "-q", cov[1], "--panel", str(asm_bed)]


def test_hand_worked_case(cli, cov, golden_dir, tmp_path):
    """tests/golden/hapnetto through the CLI: the coverage contigs are not in asm.bed, so no window reaches the panel (`subtract -a assembly`)
    and stdout is the diploid panel of the haplotype funbits alone, with the script's constants"""
    g = os.path.join(golden_dir, "hapnetto")
    names, lens, haps, fun_exp, dip_exp = hc.golden_case(golden_dir)
    assert hc.hap_fun(lens, haps) == fun_exp                                     # the restatement agrees with the hand-worked lists
    assert hc.dip_panel(lens, [], [], haps) == dip_exp
    got = cornetto_amd.panel_boring(lens, np.array(fun_exp, cornetto_amd.IVL_DT).reshape(-1), np.zeros(0, cornetto_amd.IVL_DT))
    assert [tuple(int(x) for x in r) for r in got] == dip_exp
    rc, out, err = run(cli, base_args(cov, os.path.join(g, "asm.bed")) + ["--hap", os.path.join(g, "hap1.paf"), "--hap", os.path.join(g, "hap2.paf"),
                                                                         "--hap-fun", str(tmp_path / "fun.bed")])
    assert rc == 0, err.decode()
    assert (tmp_path / "fun.bed").read_bytes() == open(os.path.join(g, "funbits.exp.bed"), "rb").read()
    assert out == open(os.path.join(g, "dip.exp.bed"), "rb").read()
    # one haplotype alone: its own funbits (README: the merged list of hap1)
    rc, out, err = run(cli, base_args(cov, os.path.join(g, "asm.bed")) + ["--hap", os.path.join(g, "hap1.paf"), "--hap-fun", str(tmp_path / "fun1.bed")])
    assert rc == 0, err.decode()
    assert (tmp_path / "fun1.bed").read_bytes() == hc.bed_text(names, hc.hap_fun(lens, haps[:1]))
    assert b"c0\t300\t1500\n" in (tmp_path / "fun1.bed").read_bytes()


def _windows(product, cov):
    """the selected fun windows of the committed coverage (host path), by coverage contig index"""
    rc, out, err = run(product, ["noboringbits", "--accel=no", cov[0], "-q", cov[1]] + COV_OPTS)
    assert rc == 0, err.decode()
    idx = {n: i for i, n in enumerate(cov[2])}
    rows = [l.split(b"\t") for l in out.splitlines()]
    return [(idx[r[0]], int(r[1]), int(r[2])) for r in rows if r[3] != b"."]


def test_cli_on_the_committed_coverage(product, cov, tmp_path):
    """`--hap` twice on the coverage fixtures with PAFs over their contigs: stdout = the restatement's diploid panel; `--dip`: stdout is the
    run without --hap and the file is the run with --hap alone; `--hap-fun` = the restatement"""
    tot, mq, names, lens = cov
    order = list(range(len(names)))[::-1]                                       # the assembly BED in another order, plus a contig of its own
    asm_names = [names[i] for i in order] + [b"only_in_assembly"]
    asm_lens = [lens[i] for i in order] + [5000]
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, l) for n, l in zip(asm_names, asm_lens)))
    _l, haps, D, F = hc.random_case(4, lens=list(asm_lens), max_queries=12, DF=(1500, 40))
    haps = (haps + haps)[:2]
    haps[1] = [(b"x" + q, c, s, e) for q, c, s, e in haps[1][::2]] or haps[0][:1]
    for k, rows in enumerate(haps):
        (tmp_path / ("hap%d.paf" % (k + 1))).write_bytes(hc.paf_text(asm_names, asm_lens, rows) + b"q9\t9\t0\t9\t+\tnot_in_assembly\t99\t1\t9\t8\t8\t60\n")
    par = ",".join(map(str, PANEL_PAR))
    common = base_args(cov, tmp_path / "asm.bed") + COV_OPTS + ["--panel-params", par]
    hap_opts = ["--hap", str(tmp_path / "hap1.paf"), "--hap", str(tmp_path / "hap2.paf"), "--hap-params", "%d,%d" % (D, F)]
    rc0, out0, err0 = run(product, common)
    assert rc0 == 0 and out0, err0.decode()
    rc1, out1, err1 = run(product, common + hap_opts + ["--hap-fun", str(tmp_path / "fun.bed")])
    assert rc1 == 0, err1.decode()
    assert b"1 rows on targets the assembly BED does not have were dropped" in err1          # dropped and counted, not an error
    fun_exp = hc.hap_fun(asm_lens, haps, D, F)
    assert (tmp_path / "fun.bed").read_bytes() == hc.bed_text(asm_names, fun_exp)
    # the diploid panel from the restatement: merged windows (create-cornetto.sh:41-47) + haplotype funbits through steps 5-9
    cmap = {i: asm_names.index(n) for i, n in enumerate(names)}
    win = ob.ivl_merge(hc._spans(_windows(product, cov)), PANEL_PAR[0])
    win = [(cmap[int(r["ctg"])], int(r["start"]), int(r["end"])) for r in win if r["end"] - r["start"] >= PANEL_PAR[1]]
    dip_exp = hc.dip_panel(asm_lens, win, [], haps, D, F, min_lowq_len=PANEL_PAR[2], extend=PANEL_PAR[3], edge_len=PANEL_PAR[4], merge_dist=PANEL_PAR[5],
                           min_ctg_len=PANEL_PAR[6])
    assert out1 == hc.bed_text(asm_names, dip_exp)
    assert out1 != out0 and len(dip_exp) > 0
    rc2, out2, err2 = run(product, common + hap_opts + ["--dip", str(tmp_path / "dip.bed")])
    assert rc2 == 0, err2.decode()
    assert out2 == out0 and (tmp_path / "dip.bed").read_bytes() == out1


def _bad(cli, cov, golden_dir, tmp_path, paf=None, args=None):
    g = os.path.join(golden_dir, "hapnetto")
    if paf is not None:
        (tmp_path / "bad.paf").write_bytes(paf)
        args = base_args(cov, os.path.join(g, "asm.bed")) + ["--hap", str(tmp_path / "bad.paf")]
    rc, out, err = run(cli, args)
    assert rc == 1 and out == b"" and err.count(b"::ERROR]") == 1, (rc, out, err.decode())
    return err


GOOD = b"q1\t500\t0\t400\t+\tc0\t3000000\t1000\t1400\t400\t400\t60\n"


def test_error_cases(cli, cov, golden_dir, tmp_path):
    """each: exit 1, nothing on stdout, one error line"""
    g = os.path.join(golden_dir, "hapnetto")
    h1 = os.path.join(g, "hap1.paf")
    assert b"Had 8." in _bad(cli, cov, golden_dir, tmp_path, GOOD + b"q1\t500\t0\t400\t+\tc0\t3000000\t1000\n")             # a line with 8 fields
    assert b"line 1: column 8 is not a number" in _bad(cli, cov, golden_dir, tmp_path, GOOD.replace(b"\t1000\t", b"\t1e3\t"))
    assert b"line 2: target end 1000 is not behind target start 1000" in _bad(cli, cov, golden_dir, tmp_path, GOOD + GOOD.replace(b"\t1400\t", b"\t1000\t"))
    assert b"column 8 is negative" in _bad(cli, cov, golden_dir, tmp_path, GOOD.replace(b"\t1000\t", b"\t-5\t"))
    assert b"no row on a contig of the assembly" in _bad(cli, cov, golden_dir, tmp_path, b"")                                # an empty PAF
    assert b"no row on a contig of the assembly" in _bad(cli, cov, golden_dir, tmp_path, GOOD.replace(b"\tc0\t", b"\tc9\t"))  # ... or one without a usable row
    two = ["noboringbits", "--accel=no", cov[0], "-q", cov[1]]
    assert b"--hap needs --panel" in _bad(cli, cov, golden_dir, tmp_path, args=two + ["--hap", h1])
    assert b"only with noboringbits" in _bad(cli, cov, golden_dir, tmp_path, args=["boringbits"] + two[1:] + ["--panel", os.path.join(g, "asm.bed"), "--hap", h1])
    assert b"--dip and --hap-fun need --hap" in _bad(cli, cov, golden_dir, tmp_path, args=two + ["--panel", os.path.join(g, "asm.bed"), "--dip", str(tmp_path / "d")])
    assert b"at most 8 haplotype PAFs" in _bad(cli, cov, golden_dir, tmp_path, args=two + ["--panel", os.path.join(g, "asm.bed")] + ["--hap", h1] * 9)
    assert b"--hap-params wants two integers" in _bad(cli, cov, golden_dir, tmp_path, args=two + ["--panel", os.path.join(g, "asm.bed"), "--hap", h1, "--hap-params", "5"])
    assert not (tmp_path / "d").exists()


def test_unknown_target_is_dropped_and_a_long_line_is_read(cli, cov, golden_dir, tmp_path):
    """a row on a target the assembly BED does not have is dropped and counted; a line of more than 1 MiB (a long cg:Z: tag) is one row; eight
    --hap options are accepted; \\r\\n line ends and a PAF of exactly nine columns are read"""
    g = os.path.join(golden_dir, "hapnetto")
    names, lens, haps, fun_exp, _dip = hc.golden_case(golden_dir)
    text = open(os.path.join(g, "hap1.paf"), "rb").read().splitlines(keepends=True)
    text[2] = text[2].rstrip(b"\n") + b"\tcg:Z:" + b"151=1X" * 200_000 + b"\n"
    assert len(text[2]) > (1 << 20)
    text.insert(1, b"h1a\t900\t0\t800\t-\tcX\t5000\t100\t900\t800\t800\t60\n")
    (tmp_path / "long.paf").write_bytes(b"".join(text))
    nine = b"".join(b"\t".join(l.split(b"\t")[:9]) + b"\r\n" for l in open(os.path.join(g, "hap2.paf"), "rb").read().splitlines())
    (tmp_path / "nine.paf").write_bytes(nine)
    args = base_args(cov, os.path.join(g, "asm.bed")) + ["--hap", str(tmp_path / "long.paf"), "--hap", str(tmp_path / "nine.paf"), "--hap-fun", str(tmp_path / "fun.bed")]
    rc, out, err = run(cli, args)
    assert rc == 0, err.decode()
    assert b"long.paf: 1 rows on targets the assembly BED does not have were dropped" in err
    assert (tmp_path / "fun.bed").read_bytes() == hc.bed_text(names, fun_exp)
    assert out == open(os.path.join(g, "dip.exp.bed"), "rb").read()
    rc, out8, err = run(cli, base_args(cov, os.path.join(g, "asm.bed")) + ["--hap", os.path.join(g, "hap1.paf"), "--hap", os.path.join(g, "hap2.paf")] * 4)
    assert rc == 0 and out8 == out, err.decode()                                    # (the same haplotypes four times: the same union)


@pytest.mark.parametrize("seed", range(30))
def test_random_pafs_against_the_restatement(product, cov, tmp_path, seed):
    lens, haps, D, F = hc.random_case(seed)
    names = hc.names_for(lens)
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, l) for n, l in zip(names, lens)))
    rng = np.random.default_rng(seed)
    args = base_args(cov, tmp_path / "asm.bed") + ["--hap-fun", str(tmp_path / "fun.bed")]
    for k, rows in enumerate(haps):
        (tmp_path / ("h%d.paf" % k)).write_bytes(hc.paf_text(names, lens, rows, rng))
        args += ["--hap", str(tmp_path / ("h%d.paf" % k))]
    if seed % 2:
        args += ["--hap-params", "%d,%d" % (D, F)]
    rc, out, err = run(product, args)
    assert rc == 0, err.decode()
    exp = hc.hap_fun(lens, haps, D, F)
    assert (tmp_path / "fun.bed").read_bytes() == hc.bed_text(names, exp), (seed, D, F)
    # no coverage contig is in this assembly: stdout is steps 5-9 on the haplotype funbits alone
    assert out == hc.bed_text(names, hc.dip_panel(lens, [], [], haps, D, F))
