"""CPU: the host side of `(no)boringbits --bam` — the oracle of tests/bam_cases.py pinned by vectors worked out by hand, cornetto_bam_header()
at every cut of a header that spans several BGZF blocks, the usage errors of the option, the host reader (`--accel=no`) against the per-base
bedgraph command on the oracle's coverage, and the device's record / CIGAR walk (csrc/bam.hpp) run on the CPU under AddressSanitizer + UBSan
(tools/sim/bam_sim.cc: a stand-alone program) over every case, seeded mutations of their record area and every truncation of a small file:
the argument for the kernels' bounds."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bam_cases as bm
import bgzf_cases as bc
import cornetto_amd
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = cornetto_amd.BAM_SCAN_TILE


def _depth(n, ivls):
    a = np.zeros(n, dtype=np.uint16)
    for s, e in ivls:
        a[s:e] += 1
    return a


# ---- the oracle, pinned by hand ----------------------------------------------------------------------------------------------------------------
def test_oracle_handworked_vectors():
    # 2S5M2D3M1I4M3H at 0-based 3: 5M covers 3..7, 2D skips 8..9, 3M covers 10..12, 1I nothing, 4M covers 13..16
    assert bm.covered(3, struct.unpack("<7I", bm.pack_ops("2S5M2D3M1I4M3H"))) == ([(3, 8), (10, 13), (13, 17)], 14)
    r = bm.oracle(bm.raw([("a", 30)], [bm.record(0, 3, "2S5M2D3M1I4M3H")]))
    assert r.status == 0 and r.n_records == 1 and r.n_counted == 1 and r.n_clamped == 0
    assert r.total[0].tolist() == [0] * 3 + [1] * 5 + [0] * 2 + [1] * 7 + [0] * 13 and r.mq[0].tolist() == r.total[0].tolist()
    assert r.recs[0]["span"] == 14 and r.recs[0]["bases"] == 12 and r.recs[0]["n_ops"] == 7
    # = and X count, N advances, P and S do neither; two reads add up; mapq 19 is in the first track only
    r = bm.oracle(bm.raw([("a", 20), ("b", 5)], [bm.record(0, 0, "1S2=1X3N1P2M", mapq=19), bm.record(0, 2, "4M", mapq=20), bm.record(1, 4, "3M")]))
    assert r.total[0].tolist() == [1, 1, 2, 1, 1, 1, 1, 1] + [0] * 12 and r.mq[0].tolist() == [0, 0, 1, 1, 1, 1] + [0] * 14
    assert r.total[1].tolist() == [0, 0, 0, 0, 1] and r.recs[2]["bases"] == 1 and r.recs[2]["span"] == 3          # cut at the contig's end
    # the four flag bits, refID -1 and a negative position
    recs = [bm.record(0, 1, "2M", flag=f) for f in (4, 0x100, 0x200, 0x400)] + [bm.record(-1, 1, "2M"), bm.record(0, -1, "3M"), bm.record(0, 1, "2M", flag=0x811)]
    r = bm.oracle(bm.raw([("a", 4)], recs))
    assert r.total[0].tolist() == [1, 2, 1, 0] and r.n_records == 7 and r.n_counted == 2
    # every contig appears, with or without reads; a contig of length 0 has no position
    r = bm.oracle(bm.raw([("a", 2), ("e", 0), ("b", 3)], []))
    assert [a.tolist() for a in r.total] == [[0, 0], [], [0, 0, 0]] and r.names == ["a", "e", "b"]
    # the long-CIGAR placeholder: with the tag the CG array is walked, without it the two operations as they stand (nothing is covered)
    r = bm.oracle(bm.raw([("a", 60)], [bm.long_record(0, 10, "20M5D20M")]))
    assert (r.total[0] == _depth(60, [(10, 30), (35, 55)])).all() and r.recs[0]["n_ops"] == 3
    r = bm.oracle(bm.raw([("a", 60)], [bm.long_record(0, 10, "20M5D20M", tag=False)]))
    assert not r.total[0].any() and r.recs[0]["span"] == 45 and r.recs[0]["n_ops"] == 2
    # the clamp: 65540 one-base reads
    r = bm.oracle(bm.raw([("a", 3)], [bm.record(0, 1, "1M", mapq=(60 if i % 2 else 0)) for i in range(65540)]))
    assert r.total[0].tolist() == [0, 65535, 0] and r.mq[0].tolist() == [0, 32770, 0] and r.n_clamped == 1


@pytest.mark.parametrize("name", sorted(bm.bad_cases()))
def test_oracle_bad_files(name):
    data, err = bm.bad_cases()[name]
    r = bm.oracle(data)
    assert r.status == -6 and r.err == err


# ---- cornetto_bam_header -------------------------------------------------------------------------------------------------------------------------
def test_bam_header_at_every_cut():
    contigs = [("contig_%d_with_a_longer_name" % i, 1000 + 17 * i) for i in range(40)] + [("e", 0)]
    text = b"@HD\tVN:1.6\n@PG\tID:x\n" * 3
    data = bm.raw(contigs, [bm.record(0, 1, "5M")], text=text)
    n_hdr = len(bm.header(contigs, text=text))
    for cut in range(len(data) + 1):
        got = cornetto_amd.bam_header(data[:cut])
        if cut < n_hdr:
            assert got is None, cut
        else:
            assert got == ([n for n, _ in contigs], [ln for _, ln in contigs], n_hdr), cut
    # the same through the blocks of a file whose header spans six of them
    blob = bc.write(data, [300] * 5)
    members = bc.inflate_members(blob)
    head, need = b"", 0
    for m in members:
        head += m
        need += 1
        if cornetto_amd.bam_header(head) is not None:
            break
    assert need == min(-(-n_hdr // 300), 6) and need > 3
    for bad in (b"BAX\1" + data[4:], b"BAM\1" + struct.pack("<i", -1) + data[8:], data[:8 + len(text)] + struct.pack("<i", -4) + data[12 + len(text):]):
        with pytest.raises(ValueError):
            cornetto_amd.bam_header(bad)
    assert bm.parse_header(data)[2] == n_hdr


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------------
ARGS = ["-w", "40", "-i", "10", "-m", "50", "-e", "20"]
PANEL_ARGS = ["-w", "1000", "-i", "100", "-m", "10000", "-e", "2000"]


def PANEL_CASE():
    """two contigs at depth ~12 with a stretch of 4 kb without reads and every third read of low mapping quality: the panel has a line"""
    contigs = [("c0", 30000), ("c1", 12000)]
    recs = [bm.record(0, s, "400M20D300M", mapq=60 if s % 3 else 5) for s in range(0, 29000, 60) if not 10000 < s < 14000]
    return contigs, recs + [bm.record(1, s, "500M") for s in range(0, 11000, 100)]


def _write_case(tmp_path, contigs, recs, sizes=None, tag="x", bump=None):
    """-> (BAM path, cov-total path, cov-mq path, oracle result).  bump: (contig, position, value) written into the bedgraphs in place of a
    clamped depth (the text readers clamp and count it themselves)"""
    data = bm.raw(contigs, recs)
    r = bm.oracle(data)
    assert r.status == 0
    paths = [str(tmp_path / (tag + ext)) for ext in (".bam", ".total.bg", ".mq.bg")]
    with open(paths[0], "wb") as f:
        f.write(bc.write(data, sizes))
    tot, mq = bm.bedgraphs(r)
    if bump:
        c, p, v = bump
        tot = tot.replace(b"%s\t%d\t%d\t65535\n" % (r.names[c].encode(), p, p + 1), b"%s\t%d\t%d\t%d\n" % (r.names[c].encode(), p, p + 1, v))
    for path, text in zip(paths[1:], (tot, mq)):
        with open(path, "wb") as f:
            f.write(text)
    return paths[0], paths[1], paths[2], r


def _strip(err):
    """the lines of stderr that are about the input (INFO lines carry timings)"""
    return [ln for ln in err.decode(errors="replace").splitlines() if "WARNING" in ln or "ERROR" in ln]


def test_usage_errors(cli, tmp_path):        # noqa: F811
    bam, tot, mq, _ = _write_case(tmp_path, [("a", 300)], [bm.record(0, 5, "100M")])
    for sub in ("noboringbits", "boringbits"):
        for extra in ([tot], ["-q", mq], ["--runs"], ["-q", mq, tot]):
            rc, out, err = run(cli, [sub, "--accel=no", "--bam", bam] + extra)
            assert rc == 1 and out == b"" and b"--bam takes the place" in err, (sub, extra, err)
    rc, out, err = run(cli, ["noboringbits", "--accel=no", "--bam", str(tmp_path / "nope.bam")])
    assert rc == 1 and out == b"" and b"Failed to open" in err
    rc, out, err = run(cli, ["noboringbits", "-h"])
    assert rc == 0 and b"--bam FILE" in out and b"--bam-mapq" in out
    for bad in ("x", "20q", "-1", "256", ""):
        rc, out, err = run(cli, ["noboringbits", "--accel=no", "--bam", bam, "--bam-mapq", bad])
        assert rc == 1 and out == b"" and b"--bam-mapq wants" in err, bad


@pytest.mark.parametrize("sub", ["noboringbits", "boringbits"])
def test_host_bam_equals_the_bedgraph_command(cli, tmp_path, sub):        # noqa: F811
    """fails on the parent commit: it has no --bam"""
    contigs, recs = bm.random_case(11, n_ctg=4, n_reads=120)
    contigs = [("c0", 900), ("empty", 0), ("c1", 400), ("c2", 64), ("c3", 1)]
    recs = [r for r in recs] + [bm.record(0, 100, "300M", mapq=60), bm.record(0, 150, "300M", mapq=3), bm.record(2, 10, "200M2D200M")]
    bam, tot, mq, r = _write_case(tmp_path, contigs, recs, sizes=[700, 333, 1000])
    assert r.n_counted > 50
    want = run(cli, [sub, "--accel=no"] + ARGS + ["-q", mq, tot])
    got = run(cli, [sub, "--accel=no"] + ARGS + ["--bam", bam])
    assert want[0] == 0 and got[0] == 0 and got[1] == want[1] and len(want[1]) > 0 and _strip(got[2]) == _strip(want[2])
    # the threshold of the second track
    r30 = bm.oracle(bm.raw(contigs, recs), min_mapq=61)
    with open(mq, "wb") as f:
        f.write(bm.bedgraphs(r30)[1])
    want = run(cli, [sub, "--accel=no"] + ARGS + ["-q", mq, tot])
    got = run(cli, [sub, "--accel=no"] + ARGS + ["--bam", bam, "--bam-mapq", "61"])
    assert got[0] == 0 and got[1] == want[1]


def test_host_bam_clamp_warning(cli, tmp_path):        # noqa: F811
    recs = [bm.record(0, 7, "1M") for _ in range(65540)] + [bm.record(0, 0, "150M")]
    bam, tot, mq, r = _write_case(tmp_path, [("a", 200)], recs, bump=(0, 7, 65541))
    assert r.n_clamped == 2
    with open(mq, "rb") as f:
        text = f.read().replace(b"a\t7\t8\t65535\n", b"a\t7\t8\t65541\n")
    with open(mq, "wb") as f:
        f.write(text)
    want = run(cli, ["noboringbits", "--accel=no"] + ARGS + ["-q", mq, tot])
    got = run(cli, ["noboringbits", "--accel=no"] + ARGS + ["--bam", bam])
    assert got[0] == 0 and got[1] == want[1] and _strip(got[2]) == _strip(want[2]) and any("2 depth values were truncated" in ln for ln in _strip(got[2]))


def test_host_bam_panel_equals_the_bedgraph_command(cli, tmp_path):        # noqa: F811
    contigs, recs = PANEL_CASE()
    bam, tot, mq, r = _write_case(tmp_path, contigs, recs)
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n.encode(), ln) for n, ln in contigs))
    panel = ["--panel", str(tmp_path / "asm.bed"), "--panel-params", "100,200,200,50,100,100,1000"]
    want = run(cli, ["noboringbits", "--accel=no", *PANEL_ARGS, "-q", mq, tot] + panel)
    got = run(cli, ["noboringbits", "--accel=no", *PANEL_ARGS, "--bam", bam] + panel)
    assert want[0] == 0 and got[0] == 0 and got[1] == want[1] and len(want[1]) > 0, (want, got)


@pytest.mark.parametrize("name", sorted(bm.bad_cases()))
def test_host_bam_bad_files(cli, tmp_path, name):        # noqa: F811
    data, err = bm.bad_cases()[name]
    p = tmp_path / "bad.bam"
    p.write_bytes(bc.write(data, [150, 90]))
    rc, out, err_text = run(cli, ["noboringbits", "--accel=no"] + ARGS + ["--bam", str(p)])
    assert rc == 1 and out == b"" and (b"record %d:" % err[1]) in err_text


def test_host_bam_bad_container(cli, tmp_path):        # noqa: F811
    data = bm.raw([("a", 300)], [bm.record(0, 5, "100M")] * 30)
    blob = bytearray(bc.write(data, [400, 400]))
    blob[len(bc.member(data[:400])) + 40] ^= 0x55          # inside the second block's deflate stream
    for name, b in (("flip", bytes(blob)), ("text", b"not a BAM at all\n" * 10), ("plain", data), ("gz", bc.write(b"no magic here " * 10)),
                    ("hdr_cut", bc.write(data[:20])), ("empty", b"")):
        p = tmp_path / (name + ".bam")
        p.write_bytes(b)
        rc, out, err = run(cli, ["noboringbits", "--accel=no"] + ARGS + ["--bam", str(p)])
        assert rc == 1 and out == b"" and b"ERROR" in err, name
    # a missing EOF block is accepted
    p = tmp_path / "noeof.bam"
    p.write_bytes(bc.write(data, [400, 400], eof=False))
    q = tmp_path / "eof.bam"
    q.write_bytes(bc.write(data, [400, 400]))
    a, b = (run(cli, ["noboringbits", "--accel=no"] + ARGS + ["--bam", str(x)]) for x in (p, q))
    assert a[0] == 0 and a[1] == b[1] and len(a[1]) > 0


# ---- the device's walk on the CPU, under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sim")
    exe = str(d / "bam_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "sim", "bam_sim.cc"), "-lz", "-o", exe])
    return exe, d


def _line(r):
    if r.status:
        return "%d %d %d %d %d" % ((r.status,) + tuple(r.err))
    return "0 0 0 0 0 %d %d %d %d %d" % (r.n_records, r.n_counted, r.n_clamped, bm.checksum(r.total), bm.checksum(r.mq))


def _run_sim(sim, datas, window=None):
    exe, d = sim
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        for x in datas:
            f.write(struct.pack("<I", len(x)) + x)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + (["--window", str(window)] if window else []) + [path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "FAIL" not in err, (p.returncode, err[-3000:])
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(datas)
    return lines


def _agree(lines, datas, names):
    for ln, x, name in zip(lines, datas, names):
        want = _line(bm.oracle(x))
        got = ln if not want.startswith("-6") else " ".join(ln.split()[:5])
        assert got == want, (name, ln, want)


def all_valid_cases():
    return bm.valid_cases(TILE)


def test_walk_under_the_sanitizers_every_case(sim):
    cases = all_valid_cases()
    names = sorted(cases)
    datas = [bm.raw(*cases[n]) for n in names]
    bad = bm.bad_cases()
    names += sorted(bad)
    datas += [bad[n][0] for n in sorted(bad)]
    _agree(_run_sim(sim, datas), datas, names)
    small = [(n, x) for n, x in zip(names, datas) if len(x) < 20000]
    for window in (1, 37, 64, 300):          # windows that cut block_size fields and records anywhere
        _agree(_run_sim(sim, [x for _, x in small], window), [x for _, x in small], [n for n, _ in small])


def test_walk_under_the_sanitizers_mutations_and_truncations(sim):
    """600 seeded changes of one to three bytes of the record area (half of them in a record's fixed fields), and a small file cut at every
    length: the walk agrees with the oracle where the file is still valid and gives the oracle's error where it is not"""
    rng = random.Random(5)
    cases = all_valid_cases()
    pool = [bm.raw(*cases[n]) for n in ("handworked", "all_ops", "zero_len", "cg_small", "cg_missing", "ops_65", "clip", "flags", "empty_contigs", "random_3")]
    datas = []
    for it in range(600):
        x = bytearray(pool[it % len(pool)])
        first = bm.parse_header(bytes(x))[2]
        for _ in range(rng.choice((1, 1, 2, 3))):
            at = first + rng.randrange(min(36, len(x) - first)) if rng.random() < 0.5 else rng.randrange(first, len(x))
            x[at] = rng.choice((0, 1, 2, 4, 0x7F, 0x80, 0xFF, x[at] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        datas.append(bytes(x))
    small = bm.raw([("a", 70), ("b", 9)], [bm.record(0, 3, "2S5M2D3M1I4M3H", aux=b"NMC\3"), bm.long_record(1, 1, "3M1D3M"), bm.record(0, 60, "20M")])
    datas += [small[:n] for n in range(len(small) + 1)]
    names = ["mutation %d" % i for i in range(600)] + ["cut at %d" % n for n in range(len(small) + 1)]
    _agree(_run_sim(sim, datas), datas, names)
    _agree(_run_sim(sim, datas, 53), datas, names)
