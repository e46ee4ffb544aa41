"""CPU: the host side of `seq --bam` — the oracle of tests/bamfq_cases.py pinned by vectors worked out by hand, the usage errors of the option,
the host reader (`--accel=no`, the product binary and the same host C under ASan + UBSan) against the oracle on every case, its composition
with `seq` on FASTQ text, and the device's size pass and text kernel (csrc/bamfq.hpp) run on the CPU under AddressSanitizer + UBSan
(tools/sim/bamfq_sim.cc: a stand-alone program) over every case at several windows and range sizes, seeded mutations of their record area
and every truncation of a small file: the argument for the kernels' bounds."""
import os
import random
import struct
import subprocess

import pytest

import bamfq_cases as fq
import bgzf_cases as bc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fq.valid_cases()
_RAW = {}


def raw_of(name):
    if name not in _RAW:
        _RAW[name] = fq.raw(CASES[name][0])
    return _RAW[name]


# ---- the oracle, pinned by hand ----------------------------------------------------------------------------------------------------------------
def test_oracle_handworked_vectors():
    # ACGTN is 1 2 4 8 15: the bytes 0x12 0x48 0xF0; qualities 0, 1, 60, 93, 94 print as ! " ] ~ ~
    rec = fq.record(b"read1", "ACGTN", bytes([0, 1, 60, 93, 94]))
    assert rec[36:42] == b"read1\0" and rec[42:45] == bytes([0x12, 0x48, 0xF0]) and rec[45:50] == bytes([0, 1, 60, 93, 94])
    r = fq.oracle(fq.raw([rec]))
    assert r.status == 0 and r.text == b"@read1\nACGTN\n+\n!\"]~~\n" and r.stats == [1, 5, 1, 5]
    # the reverse strand: reversed and complemented (N stays N), the qualities reversed
    r = fq.oracle(fq.raw([fq.record(b"read1", "ACGTN", bytes([0, 1, 60, 93, 94]), flag=0x10)]))
    assert r.text == b"@read1\nNACGT\n+\n~~]\"!\n"
    # every code: forward and complemented
    r = fq.oracle(fq.raw([fq.record(b"a", list(range(16)), bytes(16)), fq.record(b"b", list(range(16)), bytes(16), flag=0x10)]))
    assert r.text == b"@a\n=ACMGRSVTWYHKDBN\n+\n" + b"!" * 16 + b"\n@b\nNVHMDRWABSYCKGT=\n+\n" + b"!" * 16 + b"\n"
    # absent qualities, an empty read, an empty name
    r = fq.oracle(fq.raw([fq.record(b"x", "AC"), fq.record(b"e", ""), fq.record(no_name=True, bases="G", quals=b"\x05")]))
    assert r.text == b"@x\nAC\n+\n\"\"\n@e\n\n+\n\n@\nG\n+\n&\n" and r.stats == [3, 3, 3, 3]
    # 0xFF behind the first quality is a quality of 255, clamped
    assert fq.oracle(fq.raw([fq.record(b"x", "AC", b"\x05\xFF")])).text == b"@x\nAC\n+\n&~\n"
    # the length filter counts every read in the first line; secondary and supplementary records count nowhere
    recs = [fq.record(b"s", "ACG"), fq.record(b"l", "ACGTA"), fq.record(b"sec", "ACGTAC", flag=0x100), fq.record(b"sup", "ACGTAC", flag=0x800)]
    r = fq.oracle(fq.raw(recs), min_len=4)
    assert r.text == b"@l\nACGTA\n+\n\"\"\"\"\"\n" and r.stats == [2, 8, 1, 5] and [x["kept"] for x in r.recs] == [0, 1, -1, -1]
    # --duplex: dx:i:1 of an integer type only
    recs = [fq.record(b"d1", "A", aux=b"dxi\1\0\0\0"), fq.record(b"d0", "A", aux=b"dxi\0\0\0\0"), fq.record(b"dm", "A", aux=b"dxc\xFF"), fq.record(b"dz", "A", aux=b"dxZ1\0"),
            fq.record(b"none", "A"), fq.record(b"dC", "A", aux=b"qsC\7dxC\1")]
    r = fq.oracle(fq.raw(recs), duplex=True)
    assert r.text == b"@d1\nA\n+\n\"\n@dC\nA\n+\n\"\n" and r.stats == [6, 6, 2, 2]
    assert fq.summary(r, 0) == b"total reads: 6\t6 bases\t0.00 Gbases\nreads >= 0: 2\t2 bases\t0.00 Gbases\n"


@pytest.mark.parametrize("name", sorted(fq.bad_cases()))
def test_oracle_bad_files(name):
    data, err = fq.bad_cases()[name]
    r = fq.oracle(data)
    assert r.status == -6 and r.err == err
    # the text is that of the records in front of the failing one
    end = r.recs[-1]["offset"] + 4 + struct.unpack_from("<i", data, r.recs[-1]["offset"])[0] if r.recs else len(fq.HEADER)
    front = fq.oracle(data[:end])
    assert front.status == 0 and len(front.recs) == err[1] and r.text == front.text


def test_every_case_is_what_the_issue_lists():
    lens = [r["l_seq"] for r in fq.oracle(raw_of("l_seq")).recs]
    assert sorted(set(lens)) == list(fq.LENGTHS) and len(lens) == 2 * len(fq.LENGTHS)
    al = fq.oracle(raw_of("alignment"))
    starts, at = set(), 0
    for r in al.recs:
        starts.add(at % 16)
        at += r["name_len"] + 2 * r["l_seq"] + 6
    assert starts == set(range(16))
    assert len(CASES["many_small"][0]) == 10000 and max(r["l_seq"] for r in fq.oracle(raw_of("one_long")).recs) == 200001
    assert fq.oracle(raw_of("nothing_kept"), 1000).text == b"" and fq.oracle(raw_of("nothing_kept"), 0, True).text == b""
    kept = [r["kept"] for r in fq.oracle(raw_of("dx_values"), 0, True).recs]
    assert kept == [1, 0, 0] * 6 + [0, 0, 0, 1, 0]
    kept = [r["kept"] for r in fq.oracle(raw_of("dx_positions"), 0, True).recs]
    assert kept == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert [r["kept"] for r in fq.oracle(raw_of("flags"), 0, True).recs] == [-1, -1, 1, 1, -1, -1, 1, -1, 1, 1]


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, blob):
    p = tmp_path / name
    p.write_bytes(blob)
    return str(p)


def _summary_of(err):
    return b"".join(ln + b"\n" for ln in err.split(b"\n") if ln.startswith((b"total reads:", b"reads >= ")))


def test_usage_errors(cli, tmp_path):        # noqa: F811
    bam = _write(tmp_path, "x.bam", fq.bam([fq.record(b"r", "ACGT")]))
    fastq = _write(tmp_path, "x.fastq", b"@r\nACGT\n+\n!!!!\n")
    rc, out, err = run(cli, ["seq", "--accel=no", "--bam", bam, fastq])
    assert rc == 1 and out == b"" and b"--bam takes the place" in err
    rc, out, err = run(cli, ["seq", "--duplex", fastq])
    assert rc == 1 and out == b"" and b"--duplex: only with --bam" in err
    rc, out, err = run(cli, ["seq", "--accel=no", "--bam", str(tmp_path / "nope.bam")])
    assert rc == 1 and out == b"" and b"Failed to open" in err
    rc, out, err = run(cli, ["seq", "-h"])
    assert rc == 0 and out.startswith(b"Usage") and b"--bam FILE" in out and b"--duplex" in out and out.count(b"(extension)") == 2
    rc, out, err = run(cli, ["seq"])
    assert rc == 1 and out == b"" and b"Usage" in err
    # seq without --bam is what it was
    rc, out, err = run(cli, ["seq", "-m", "0", fastq])
    assert rc == 0 and out == b"@r\nACGT\n+\n!!!!\n" and _summary_of(err) == b"total reads: 1\t4 bases\t0.00 Gbases\nreads >= 0: 1\t4 bases\t0.00 Gbases\n"


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_reader_equals_the_oracle(cli, tmp_path, name):        # noqa: F811
    """fails on the parent commit: it has no --bam"""
    recs, runs = CASES[name]
    bam = _write(tmp_path, "c.bam", fq.bam(recs, sizes=[700, 333, 1000]))
    for min_len, duplex in runs:
        want = fq.oracle(raw_of(name), min_len, duplex)
        rc, out, err = run(cli, ["seq", "--accel=no", "-m", str(min_len), "--bam", bam] + (["--duplex"] if duplex else []))
        assert rc == 0 and out == want.text and _summary_of(err) == fq.summary(want, min_len), (min_len, duplex, err[-500:])


def test_host_reader_seams(cli, tmp_path):        # noqa: F811
    recs, sizes = fq.seam_case()
    bam = _write(tmp_path, "s.bam", fq.bam(recs, sizes=sizes))
    for duplex in (False, True):
        want = fq.oracle(fq.raw(recs), 0, duplex)
        rc, out, err = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", bam] + (["--duplex"] if duplex else []))
        assert rc == 0 and out == want.text and len(want.text) > 0 and _summary_of(err) == fq.summary(want, 0)


def test_composition_with_seq(cli, tmp_path):        # noqa: F811
    """`seq -m N` on the text of `-m 0` is the text of `-m N`"""
    for name, n in (("l_seq", 17), ("many_small", 20), ("flags", 31)):
        all_text = fq.oracle(raw_of(name), 0).text
        want = fq.oracle(raw_of(name), n)
        fastq = _write(tmp_path, name + ".fastq", all_text)
        rc, out, err = run(cli, ["seq", "-m", str(n), fastq])
        assert rc == 0 and out == want.text and _summary_of(err) == fq.summary(want, n)


@pytest.mark.parametrize("name", sorted(fq.bad_cases()))
def test_host_reader_bad_files(cli, tmp_path, name):        # noqa: F811
    data, err = fq.bad_cases()[name]
    want = fq.oracle(data)
    bam = _write(tmp_path, "bad.bam", bc.write(data, [150, 90]))
    rc, out, err_text = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", bam])
    assert rc == 1 and out == want.text and (b"record %d:" % err[1]) in err_text and b"total reads" not in err_text


def test_host_reader_bad_container(cli, tmp_path):        # noqa: F811
    data = fq.raw([fq.record(b"r%d" % k, "ACGT" * 10, bytes(40)) for k in range(30)])
    blob = bytearray(bc.write(data, [400, 400]))
    blob[len(bc.member(data[:400])) + 40] ^= 0x55          # inside the second block's deflate stream
    for name, b in (("flip", bytes(blob)), ("text", b"not a BAM at all\n" * 10), ("plain", data), ("gz", bc.write(b"no magic here " * 10)), ("hdr_cut", bc.write(data[:8])),
                    ("empty", b"")):
        rc, out, err = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", _write(tmp_path, name + ".bam", b)])
        assert rc == 1 and b"ERROR" in err and fq.oracle(data).text.startswith(out), name
    a = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", _write(tmp_path, "noeof.bam", bc.write(data, [400, 400], eof=False))])
    assert a[0] == 0 and a[1] == fq.oracle(data).text          # a missing EOF block is accepted


# ---- the device's size pass and text kernel on the CPU, under the sanitizers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamfq_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "bamfq_sim"])
    return os.path.join(ROOT, "cornetto_amd", "bamfq_sim"), d


def _run_sim(sim, datas, args=()):
    exe, d = sim
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        for x in datas:
            f.write(struct.pack("<I", len(x)) + x)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + [str(a) for a in args] + [path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (p.returncode, err[-3000:])
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(datas)
    return lines


def test_sim_every_case_window_and_range(sim):
    bad = fq.bad_cases()
    for name in sorted(CASES):
        data = raw_of(name)
        for min_len, duplex in CASES[name][1]:
            want = fq.line(fq.oracle(data, min_len, duplex))
            flags = ["--min-len", min_len] + (["--duplex"] if duplex else [])
            longest = max(n for _, n in fq.record_sizes(data))
            small = len(data) < 100000
            for window in ([0, 37, 300, 1000] if small else [0, 70000]):
                for rng in ((1, 16, 48, 4096) if small or not window else (4096,)):
                    if rng == 1 and not small:
                        continue
                    got = _run_sim(sim, [data], flags + ["--window", window, "--range", rng])[0]
                    assert got == want, (name, min_len, duplex, window, rng, longest)
    names = sorted(bad)
    datas = [bad[n][0] for n in names]
    for window in (0, 1, 53, 300):
        for rng in (1, 16, 48, 4096):
            got = _run_sim(sim, datas, ["--window", window, "--range", rng])
            assert got == [fq.line(fq.oracle(x)) for x in datas], (window, rng)
    recs, _ = fq.seam_case()
    for duplex in ([], ["--duplex"]):
        assert _run_sim(sim, [fq.raw(recs)], ["--window", 97, "--range", 48] + duplex)[0] == fq.line(fq.oracle(fq.raw(recs), 0, bool(duplex)))


def test_sim_mutations_and_truncations(sim):
    """600 seeded changes of one to three bytes of the record area (half of them in a record's fixed fields), and a small file cut at every
    length: the simulation agrees with the oracle where the file is still valid and gives the oracle's error and text where it is not"""
    rng = random.Random(5)
    pool = [raw_of(n) for n in ("l_seq", "names", "nibbles", "quals", "dx_values", "dx_positions", "flags", "alignment")]
    datas = []
    for it in range(600):
        x = bytearray(pool[it % len(pool)])
        first = len(fq.HEADER)
        sizes = fq.record_sizes(bytes(pool[it % len(pool)]))
        for _ in range(rng.choice((1, 1, 2, 3))):
            off, n = rng.choice(sizes)
            at = off + rng.randrange(36) if rng.random() < 0.5 else rng.randrange(first, len(x))
            x[at] = rng.choice((0, 1, 2, 4, 0x7F, 0x80, 0xFF, x[at] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        datas.append(bytes(x))
    small = fq.raw([fq.record(b"ab", "ACGTACGTACGTACGTACG", bytes(range(19)), aux=b"RGZg\0dxc\1"), fq.record(b"c", "ACGTA", flag=0x14, aux=b"dxi\1\0\0\0"),
                    fq.record(no_name=True, bases="ACGTACGTACGTACGTAC", quals=bytes(18), flag=0x10)])
    datas += [small[:n] for n in range(len(small) + 1)]
    for duplex in (False, True):
        want = [fq.line(fq.oracle(x, 0, duplex)) for x in datas]
        for args in (["--range", 48], ["--window", 53, "--range", 16]):
            got = _run_sim(sim, datas, args + (["--duplex"] if duplex else []))
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, (i, duplex, args)
