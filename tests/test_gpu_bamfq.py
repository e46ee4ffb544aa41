"""GPU: the FASTQ text of a BAM on the device (csrc/bamfq.hip, cornetto_bamfq_*) and `seq --bam`, against the oracle of tests/bamfq_cases.py with
exact equality: text, both summary counts, the record table, the status and the error record.

Every case runs at three windows — the smallest that holds its largest record and one block more, a little more than twice that, and one
that holds the file — and its text is fetched in slabs of 16, 48 and 4096 bytes and as a whole, so gets cut records anywhere: all four at
the smallest window, the last two at the others (a text above 64 KiB — the 10 000 small records, the reads of 200 000 bases — takes the
16- and 48-byte slabs, tens of thousands of launches, in its first run only and 65 521-byte ones in the others).  Every bad file here went through
tools/sim/bamfq_sim.cc under the host sanitizers first (tests/test_bamfq_host.py): they are refused by checks that read inside the text."""
import os
import subprocess

import numpy as np
import pytest

import bamfq_cases as fq
import bgzf_cases as bc
import cornetto_amd
from cornetto_amd import AccelError, BamFormatError

pytestmark = pytest.mark.gpu
CASES = fq.valid_cases()
_ORACLE = {}


def oracle_of(name, min_len, duplex):
    key = (name, min_len, duplex)
    if key not in _ORACLE:
        _ORACLE[key] = fq.oracle(fq.raw(CASES[name][0]), min_len, duplex)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def same(got, want):
    text, stats, recs = got
    assert text == want.text, (len(text), len(want.text), next((i for i, (a, b) in enumerate(zip(text, want.text)) if a != b), None))
    assert stats == want.stats
    assert len(recs) == len(want.recs)
    for k in ("offset", "l_seq", "flag", "name_len", "kept"):
        assert np.array_equal(recs[k], np.array([r[k] for r in want.recs], dtype=np.int64)), k


def block_size(data):
    return 1000 if len(data) < 100000 else 60000


def windows(data, sizes):
    longest = max((n for _, n in fq.record_sizes(data)), default=0)
    least = longest + max(sizes)
    return [least, 2 * least + 17, len(data) + max(sizes)]


def slabs(want, first_run):
    return (16, 48, 4096, None) if len(want.text) <= 65536 or first_run else (65521, 4096, None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(acc, name):
    recs, runs = CASES[name]
    data = fq.raw(recs)
    sizes = [block_size(data)] * (len(data) // block_size(data) + 1)
    blob = bc.write(data, sizes)
    for k, (min_len, duplex) in enumerate(runs):
        want = oracle_of(name, min_len, duplex)
        for i, window in enumerate(windows(data, sizes)):
            for slab in (slabs(want, k == 0) if i == 0 else slabs(want, k == 0)[-2:]):
                same(acc.bam_fastq(blob, min_len, duplex, window=window, slab=slab), want)
    min_len, duplex = runs[0]
    same(acc.bam_fastq(blob, min_len, duplex, window=windows(data, sizes)[1], feeds=3), oracle_of(name, min_len, duplex))       # the tail is carried across feeds


def test_bgzf_seams(acc):
    recs, sizes = fq.seam_case()
    data = fq.raw(recs)
    blob = bc.write(data, sizes)
    longest = max(n for _, n in fq.record_sizes(data))
    for duplex in (False, True):
        want = fq.oracle(data, 0, duplex)
        for window in (longest + max(sizes), 3 * max(sizes) + longest, 1 << 20):       # every window ends at a block seam: inside a field
            for slab in (16, 48, None):
                same(acc.bam_fastq(blob, 0, duplex, window=window, slab=slab), want)


def test_one_handle_two_files(acc):
    """two different files one after the other on one handle equal the same files on fresh handles: every table and counter the stage reads is
    written in the same feed"""
    jobs = [("many_small", 20, False, 70000, 4096), ("dx_values", 0, True, 2000, 48), ("one_long", 30000, False, 400000, None), ("flags", 0, True, 1500, 16)]
    blobs = {n: fq.bam(CASES[n][0], sizes=[block_size(fq.raw(CASES[n][0]))] * 2000) for n, *_ in jobs}
    for order in (jobs, jobs[::-1]):
        for name, min_len, duplex, window, slab in order:
            same(acc.bam_fastq(blobs[name], min_len, duplex, window=window, slab=slab), oracle_of(name, min_len, duplex))
    for name, min_len, duplex, window, slab in jobs[:2]:
        fresh = cornetto_amd.Accel(0)
        try:
            same(fresh.bam_fastq(blobs[name], min_len, duplex, window=window, slab=slab), oracle_of(name, min_len, duplex))
        finally:
            fresh.close()


def test_record_larger_than_the_window(acc):
    recs = CASES["one_long"][0]
    blob = fq.bam(recs, sizes=[60000] * 40)
    with pytest.raises(AccelError) as e:
        acc.bam_fastq(blob, 0, False, window=200000)
    assert e.value.status == -4


# ---- bad files: each kind returns its status, its error record and the text in front of it --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fq.bad_cases()))
def test_bad_files(acc, name):
    data, err = fq.bad_cases()[name]
    want = fq.oracle(data)
    for sizes, window, slab in ((None, None, None), ([150, 90, 120], 400, 16), ([150, 90, 120], 1000, 48)):
        with pytest.raises(BamFormatError) as e:
            acc.bam_fastq(bc.write(data, sizes), 0, False, window=window, slab=slab)
        assert (e.value.kind, e.value.record, e.value.a, e.value.b) == err, (sizes, window)
        same((e.value.text, e.value.stats, e.value.records), want)


def test_bad_containers(acc):
    recs = [fq.record(b"r%d" % k, "ACGT" * 10, bytes(40)) for k in range(30)]
    data = fq.raw(recs)
    whole = [(off, n) for off, n in fq.record_sizes(data) if off + n <= 400]
    blob = bytearray(bc.write(data, [400, 400]))
    blob[len(bc.member(data[:400])) + 40] ^= 0x55          # inside the second block's deflate stream
    for window in (None, 900):
        with pytest.raises(BamFormatError) as e:
            acc.bam_fastq(bytes(blob), 0, False, window=window)
        assert (e.value.kind, e.value.record, e.value.a) == (fq.E_BGZF, len(whole), 1)
        assert e.value.text == fq.oracle(data[:whole[-1][0] + whole[-1][1]]).text          # the records in front of the block
    for junk, kind in ((b"not a BAM at all\n" * 10, 7), (bc.write(b"no magic here " * 10), 7), (bc.write(data[:8]), 2), (b"", 2)):
        with pytest.raises(BamFormatError) as e:
            acc.bam_fastq(junk)
        assert e.value.kind == kind
    same(acc.bam_fastq(bc.write(data, [400, 400], eof=False)), fq.oracle(data))          # a missing EOF block is accepted


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


def lines_of(err):
    """the summary lines, and the WARNING and ERROR lines without the name of the function that printed them"""
    out = []
    for ln in err.decode(errors="replace").splitlines():
        if ln.startswith(("total reads:", "reads >= ")):
            out.append(ln)
        elif "WARNING]" in ln or "ERROR]" in ln:
            out.append(ln.split("]", 1)[1])
    return out


@pytest.mark.parametrize("name", ["dx_positions", "many_small"])
def test_cli_equals_the_host_reader(cli, tmp_path, name):
    """the default window and slab, then small ones that cut the file into several windows and every window's text into many slabs"""
    small = {"CORNETTO_BAM_WINDOW": "70000", "CORNETTO_EMIT_SLAB": "4099", "CORNETTO_CLI_TRACE": "1"}
    recs, runs = CASES[name]
    p = tmp_path / (name + ".bam")
    p.write_bytes(fq.bam(recs, sizes=[5000] * 400))
    for min_len, duplex in runs:
        args = ["seq", "-m", str(min_len), "--bam", str(p)] + (["--duplex"] if duplex else [])
        want = run(cli, args + ["--accel=no"])
        assert want[0] == 0 and want[1] == oracle_of(name, min_len, duplex).text and lines_of(want[2]) == fq.summary(oracle_of(name, min_len, duplex), min_len).decode().splitlines()
        for env in ({}, small):
            got = run(cli, args, env)
            assert got[0] == 0 and got[1] == want[1] and lines_of(got[2]) == lines_of(want[2]), (name, min_len, duplex, env, got[2][-1500:])
    assert b"[cli trace] seq --bam: feed" in got[2] and b"[cli trace] device 0 opened" in got[2]


@pytest.mark.parametrize("name", ["short_block", "cut_record", "fields_l_seq", "refid_low", "first_error_wins"])
def test_cli_bad_files_equal_the_host_reader(cli, tmp_path, name):
    """one file per kind (the binding has taken all of them above): the text in front of the failing record, the one ERROR line, status 1"""
    data, err = fq.bad_cases()[name]
    p = tmp_path / (name + ".bam")
    p.write_bytes(bc.write(data, [150, 90, 120]))
    args = ["seq", "-m", "0", "--bam", str(p)]
    want = run(cli, args + ["--accel=no"])
    assert want[0] == 1 and want[1] == fq.oracle(data).text and b"total reads" not in want[2]
    got = run(cli, args, {"CORNETTO_BAM_WINDOW": "400", "CORNETTO_EMIT_SLAB": "16"})
    assert got[0] == 1 and got[1] == want[1] and lines_of(got[2]) == lines_of(want[2]) and len(lines_of(got[2])) == 1, (name, got[2][-1500:])


def test_cli_no_bam(cli, tmp_path):
    for junk in (bc.write(b"no magic here " * 10), b""):
        p = tmp_path / "junk.bam"
        p.write_bytes(junk)
        got, want = run(cli, ["seq", "--bam", str(p)]), run(cli, ["seq", "--bam", str(p), "--accel=no"])
        assert got[0] == 1 and got[1] == b"" and lines_of(got[2]) == lines_of(want[2]) and len(lines_of(got[2])) == 1


def test_cli_record_larger_than_the_window(cli, tmp_path):
    recs = CASES["one_long"][0]
    p = tmp_path / "long.bam"
    p.write_bytes(fq.bam(recs, sizes=[60000] * 40))
    args = ["seq", "-m", "0", "--bam", str(p)]
    a, b = run(cli, args), run(cli, args, {"CORNETTO_BAM_WINDOW": "200000"})       # the second one reads the rest of the file on the host
    assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == oracle_of("one_long", 0, False).text
    assert [ln for ln in lines_of(a[2]) if "WARNING" not in ln] == lines_of(a[2]) == fq.summary(oracle_of("one_long", 0, False), 0).decode().splitlines()
    assert b"on the host" in b[2] and b"on the host" not in a[2] and lines_of(b[2])[-2:] == lines_of(a[2])
    for bad in ("0", "-5", "12x", str(0x80000001)):
        rc, out, err = run(cli, args, {"CORNETTO_BAM_WINDOW": bad})
        assert rc == 1 and out == b"" and b"CORNETTO_BAM_WINDOW wants" in err, bad
