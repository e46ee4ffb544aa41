"""GPU: both coverage tracks from a BAM on the device (csrc/bam.hip, cornetto_bamdepth_*) and `(no)boringbits --bam`, against the oracle of
tests/bam_cases.py with exact equality, position by position (cornetto_cov_download).

The shapes are the smallest at which each part can go wrong: BGZF and window seams 1, 2 and 3 bytes into a block_size field, windows of two
and three blocks, CIGARs of 63 / 64 / 65 / 128 / 200 operations (a batch is 64) and of 70 000 behind a CG tag, reads cut at a contig's end,
contigs and read ends at and around the scan tile (T = BAM_SCAN_TILE), empty contigs, the clamp at 65 535.  Every bad file here went through
tools/sim/bam_sim.cc under the host sanitizers first (tests/test_bam_host.py): they are inputs to the validation."""
import os
import subprocess

import numpy as np
import pytest

import bam_cases as bm
import bgzf_cases as bc
import cornetto_amd
from cornetto_amd import BAM_SCAN_TILE as T, AccelError, BamFormatError

pytestmark = pytest.mark.gpu
CASES = bm.valid_cases(T)
_ORACLE = {}


def oracle_of(name):
    if name not in _ORACLE:
        _ORACLE[name] = bm.oracle(bm.raw(*CASES[name]))
    return _ORACLE[name]


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def check(acc, blob, want, **kw):
    cov, names, n_rec, n_cnt, n_cl = acc.bam_depth(blob, **kw)
    try:
        assert names == want.names and list(cov.lens) == want.lens
        assert (n_rec, n_cnt, n_cl) == (want.n_records, want.n_counted, want.n_clamped)
        for c in range(len(names)):
            d, q = acc.cov_download(cov, c)
            assert np.array_equal(d, want.total[c]), (c, np.flatnonzero(d != want.total[c])[:5])
            assert np.array_equal(q, want.mq[c]), (c, np.flatnonzero(q != want.mq[c])[:5])
    finally:
        cov.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(acc, name):
    check(acc, bm.bam(*CASES[name]), oracle_of(name))


def seam_sizes(data, k, every=150):
    """block sizes whose seams fall k bytes into the block_size field of a record, about `every` bytes apart"""
    cuts, last = [], 0
    for off, n in bm.record_sizes(data):
        if off + k - last >= every:
            cuts.append(off + k)
            last = off + k
    return [b - a for a, b in zip([0] + cuts, cuts)], max(n for _, n in bm.record_sizes(data))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("per_window", [2, 3])
def test_seams_inside_block_size(acc, k, per_window):
    name = "random_3"
    data = bm.raw(*CASES[name])
    sizes, longest = seam_sizes(data, k)
    assert len(sizes) > 8
    sizes += [150] * (1 + (len(data) - sum(sizes)) // 150)          # the rest in small blocks too
    blob = bc.write(data, sizes)
    check(acc, blob, oracle_of(name))                                # one window: the seams are BGZF seams only
    window = max(per_window * max(sizes), longest + max(sizes))      # every window ends at a block seam: inside a block_size field
    check(acc, blob, oracle_of(name), window=window)
    check(acc, blob, oracle_of(name), window=window, feeds=3)        # the tail is carried across feeds as well


def test_record_larger_than_the_window(acc, cli, tmp_path):
    contigs = [("a", 5000)]
    recs = [bm.record(0, 5, "100M"), bm.record(0, 50, [(1, "M"), (1, "I")] * 400 + [(100, "M")]), bm.record(0, 7, "300M")]
    blob = bm.bam(contigs, recs, sizes=[200] * 40)
    want = bm.oracle(bm.raw(contigs, recs))
    check(acc, blob, want, window=4000)
    with pytest.raises(AccelError) as e:
        acc.bam_depth(blob, window=3000)
    assert e.value.status == -4
    p = tmp_path / "big.bam"
    p.write_bytes(blob)
    args = ["noboringbits", "-w", "40", "-i", "10", "-m", "50", "-e", "20", "--bam", str(p)]
    a, b = run(cli, args), run(cli, args, {"CORNETTO_BAM_WINDOW": "3000"})       # the second one reads the file on the host
    assert a[0] == 0 and b[0] == 0 and a[1] == b[1] and len(a[1]) > 0
    assert b"reading the file on the host" in b[2] and b"reading the file on the host" not in a[2]          # the fallback says so
    for bad in ("0", "-5", "12x", str(0xF0000001)):
        rc, out, err = run(cli, args, {"CORNETTO_BAM_WINDOW": bad})
        assert rc == 1 and out == b"" and b"CORNETTO_BAM_WINDOW wants" in err, bad


def test_clamp(acc):
    recs = [bm.record(0, 70, "1M", mapq=(60 if i % 2 else 0)) for i in range(65540)] + [bm.record(0, 69, "3M"), bm.record(1, 0, "5M")]
    contigs = [("a", 200), ("b", 7)]
    want = bm.oracle(bm.raw(contigs, recs))
    assert want.n_clamped == 1 and want.total[0][70] == 65535 and want.mq[0][70] == 32771
    check(acc, bm.bam(contigs, recs), want)
    check(acc, bm.bam(contigs, recs), want, window=200000)


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_random_differential(acc, seed):
    contigs, recs = bm.random_case(seed, n_ctg=1 + seed % 3 * 4, n_reads=400)
    want = bm.oracle(bm.raw(contigs, recs))
    check(acc, bm.bam(contigs, recs, sizes=[5000 + seed] * 50), want, window=20000, min_mapq=20)
    want7 = bm.oracle(bm.raw(contigs, recs), min_mapq=60)
    check(acc, bm.bam(contigs, recs), want7, min_mapq=60)


def test_fixture_records(acc, golden_dir):
    """the reference's example.bam (50 long reads, up to 180 operations, 2.5 to 38 KB a record, over 17 blocks): framing and fields"""
    with open(os.path.join(golden_dir, "example.bam"), "rb") as f:
        blob = f.read()
    want = bm.oracle(b"".join(bc.inflate_members(blob)), depth=False)
    assert want.status == 0 and want.n_records == 50 and len(bc.members(blob)) >= 17
    for window in (None, 131072):
        got = acc.bam_records(blob, window=window)
        assert len(got) == 50
        for g, w in zip(got, want.recs):
            assert {k: int(g[k]) for k in w} == w


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def run(cli, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return p.returncode, p.stdout, p.stderr


def warnings(err):
    """the WARNING and ERROR lines without the name of the function that printed them"""
    return [ln.split("]", 1)[1] for ln in err.decode(errors="replace").splitlines() if "WARNING]" in ln or "ERROR]" in ln]


def test_cli_equals_the_bedgraph_command(cli, tmp_path):
    contigs = [("c0", 30000), ("empty", 0), ("c1", 12000), ("one", 1)]
    recs = [bm.record(0, s, "400M20D300M", mapq=60 if s % 3 else 5) for s in range(0, 29000, 60) if not 10000 < s < 14000]
    recs += [bm.record(2, s, "500M") for s in range(0, 11000, 100)] + [bm.record(0, 777, "1M", mapq=0) for _ in range(65600)]
    data = bm.raw(contigs, recs)
    r = bm.oracle(data)
    assert r.n_clamped == 1
    tot, mq = bm.bedgraphs(r)
    tot = tot.replace(b"c0\t777\t778\t65535\n", b"c0\t777\t778\t65599\n")          # the text reader clamps and counts it itself
    paths = {}
    for k, v in (("bam", bc.write(data)), ("tot", tot), ("mq", mq), ("bed", b"".join(b"%s\t0\t%d\n" % (n.encode(), ln) for n, ln in contigs if ln))):
        paths[k] = str(tmp_path / k)
        with open(paths[k], "wb") as f:
            f.write(v)
    opts = ["-w", "1000", "-i", "100", "-m", "10000", "-e", "2000"]
    for sub, extra in (("noboringbits", []), ("boringbits", []), ("noboringbits", ["--panel", paths["bed"], "--panel-params", "300,2000,500,700,3000,2500,4000"])):
        want = run(cli, [sub] + opts + extra + ["-q", paths["mq"], paths["tot"]])
        assert want[0] == 0 and len(want[1]) > 0, want
        for env in ({}, {"CORNETTO_BAM_WINDOW": "140000"}, {"CORNETTO_DEVICES": "0,0"}):
            got = run(cli, [sub] + opts + extra + ["--bam", paths["bam"]], env)
            assert got[0] == 0 and got[1] == want[1] and warnings(got[2]) == warnings(want[2]), (sub, extra, env, got[2][-2000:])
    assert any("1 depth values were truncated" in ln for ln in warnings(want[2]))


def test_cli_reads_the_bam_on_the_first_listed_device(cli, tmp_path):
    """CORNETTO_DEVICES = <last device>,0: the first handle the CLI opens is the last device's (on a box with one device both are 0), the
    finished coverage is dealt to both (cornetto_cov_shard) and the output is the one-device output"""
    last = cornetto_amd.lib().cornetto_accel_device_count() - 1
    contigs = [("c0", 30000), ("c1", 12000), ("c2", 15000)]
    recs = [bm.record(c, s, "400M20D300M", mapq=60 if s % 3 else 5) for c, (_, ln) in enumerate(contigs) for s in range(0, ln - 1000, 70) if not 10000 < s < 14000]
    p = tmp_path / "d.bam"
    p.write_bytes(bm.bam(contigs, recs))
    args = ["noboringbits", "-w", "1000", "-i", "100", "-m", "10000", "-e", "2000", "--bam", str(p)]
    one = run(cli, args, {"CORNETTO_CLI_TRACE": "1"})
    two = run(cli, args, {"CORNETTO_CLI_TRACE": "1", "CORNETTO_DEVICES": "%d,0" % last})
    opened = lambda err: [int(ln.split()[3]) for ln in err.decode(errors="replace").splitlines() if ln.startswith("[cli trace] device")]
    assert one[0] == 0 and two[0] == 0 and two[1] == one[1] and len(one[1]) > 0
    assert opened(one[2]) == [0] and opened(two[2])[0] == last, two[2][-1500:]
    assert b"Found regions on 2 devices" in two[2] and b"Found regions on" not in one[2].replace(b"Found regions in", b"")


# ---- bad files: each kind returns its status and its error record -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bm.bad_cases()))
def test_bad_files(acc, name):
    data, err = bm.bad_cases()[name]
    for sizes, window in ((None, None), ([150, 90, 120], 400)):
        with pytest.raises(BamFormatError) as e:
            acc.bam_depth(bc.write(data, sizes), window=window)
        assert (e.value.kind, e.value.record, e.value.a, e.value.b) == err, (sizes, window)


def test_bad_containers(acc):
    data = bm.raw([("a", 300)], [bm.record(0, 5, "100M")] * 30)
    whole = sum(1 for off, n in bm.record_sizes(data) if off + n <= 400)
    blob = bytearray(bc.write(data, [400, 400]))
    blob[len(bc.member(data[:400])) + 40] ^= 0x55          # inside the second block's deflate stream
    for window in (None, 900):
        with pytest.raises(BamFormatError) as e:
            acc.bam_depth(bytes(blob), window=window)
        assert (e.value.kind, e.value.record, e.value.a) == (bm.E_BGZF, whole, 1)
    for junk, kind in ((b"not a BAM at all\n" * 10, 7), (bc.write(b"no magic here " * 10), 7), (bc.write(data[:20]), 2), (b"", 2)):
        with pytest.raises(BamFormatError) as e:
            acc.bam_depth(junk)
        assert e.value.kind == kind
    want = bm.oracle(data)
    check(acc, bc.write(data, [400, 400], eof=False), want)          # a missing EOF block is accepted
