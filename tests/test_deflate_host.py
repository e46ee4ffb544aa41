"""CPU: the BGZF encoder of `seq --bam --bgzf` — the device's encoder (csrc/deflate.hpp) run on the CPU under AddressSanitizer + UBSan
(tools/sim/deflate_sim.cc: a stand-alone program) over every payload of tests/deflate_cases.py, every member checked with zlib and the size
conditions pinned; and the host path of the CLI (`--accel=no`: one small writer on zlib), the product binary and the sanitized build of the
same host C, against the plain output of the same command."""
import gzip
import os
import subprocess
import zlib

import pytest

import bamfq_cases as fq
import bgzf_cases as bc
import cornetto_amd
import deflate_cases as dc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOADS = dc.payloads()
CASES = fq.valid_cases()


# ---- the payloads keep their shapes -------------------------------------------------------------------------------------------------------------
def test_payloads_are_what_the_encoder_must_meet():
    assert {len(PAYLOADS["len_%d" % n][0]) for n in (0, 1, 2, 63, 64, 65, 65279, 65280, 65281, 130560)} == {0, 1, 2, 63, 64, 65, 65279, 65280, 65281, 130560}
    assert set(PAYLOADS["one_value"][0]) == {ord("G")} and sorted(PAYLOADS["all_256"][0]) == list(range(256))
    acgt = PAYLOADS["acgt"][0]
    assert set(acgt) == set(b"ACGT") and all(15500 < acgt.count(c) < 17100 for c in b"ACGT")
    # the Huffman tree of the Fibonacci counts is 21 deep; the counts of the second block are Fibonacci together with the end-of-block symbol:
    # the tree the encoder builds for it is 21 deep, and the limit of 15 bits must act
    fib, fib_eob = PAYLOADS["fibonacci"][0], PAYLOADS["fibonacci_eob"][0]
    counts = sorted(fib.count(bytes([c])) for c in set(fib))
    assert len(fib) == 46367 and len(counts) == 22 and counts[:5] == [1, 1, 2, 3, 5] and counts[-1] == 17711 and dc.huffman_depth(counts) == 21
    assert len(fib_eob) == 46366 and dc.huffman_depth([fib_eob.count(bytes([c])) for c in set(fib_eob)] + [1]) == 21
    # random bytes do not deflate; zlib's Huffman-only stream of the FASTQ-like block is below its level 1 (what the size condition rests on)
    z = zlib.compressobj(9, zlib.DEFLATED, -15)
    assert len(z.compress(PAYLOADS["random"][0]) + z.flush()) > dc.MEMBER
    text = PAYLOADS["fastq"][0]
    h = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    one = zlib.compressobj(1, zlib.DEFLATED, -15)
    assert len(h.compress(text) + h.flush()) < len(one.compress(text) + one.flush())
    data, at = PAYLOADS["odd_offset"]
    assert at % 2 == 1 and len(data) - at > dc.MEMBER
    for s in (61, 62, 63, 64):
        d = PAYLOADS["run4_at_%d" % s][0]
        assert d[64 + s:64 + s + 4] == b"N" * 4 and d.count(b"N") == 4 and all(a != b for a, b in zip(d, d[1:]) if a != ord("N"))


# ---- the encoder under the sanitizers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim_out(tmp_path_factory):
    """deflate_sim over every payload: {name: the chain it wrote}"""
    d = tmp_path_factory.mktemp("deflate_sim")
    exe = str(d / "deflate_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "sim", "deflate_sim.cc"), "-lz", "-o", exe])
    files = []
    for name, (data, at) in sorted(PAYLOADS.items()):
        (d / name).write_bytes(data[at:])
        files.append(str(d / name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "FAIL" not in err, (p.returncode, p.stdout[-500:], err[-3000:])
    words = p.stdout.decode().splitlines()[-1].split()
    assert int(words[1]) == sum((len(data) - at + dc.MEMBER - 1) // dc.MEMBER for data, at in PAYLOADS.values()) and int(words[3]) == 0
    return {name: (d / (name + ".bgzf")).read_bytes() for name in PAYLOADS}


@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_encoder_under_the_sanitizers_against_zlib(sim_out, name):
    """every member inflates under zlib to its piece of the payload with the right CRC-32 and ISIZE, is at most 65311 bytes, the chain is
    one cornetto_bgzf_scan() accepts, and the size conditions hold"""
    data, at = PAYLOADS[name]
    payload, blob = data[at:], sim_out[name]
    sizes = dc.check_chain(blob, payload)
    dc.check_sizes(name, sizes, payload)
    blocks, resume, broken = cornetto_amd.bgzf_scan(blob)
    assert not broken and resume == len(blob) and len(blocks) == len(sizes) and int(blocks["n_dst"].sum()) == len(payload)
    assert gzip.decompress(blob + bc.EOF_BLOCK) == payload


def test_runs_are_matches(sim_out):
    """a run of 4 or more bytes of one value is a literal and distance-1 matches, whatever tile it begins in; shorter runs are literals"""
    for s in (61, 62, 63, 64):
        blob = sim_out["run4_at_%d" % s]
        (_, _, pay, n_pay, _, _), = bc.members(blob)
        w = bc.walk(blob[pay:pay + n_pay])
        assert w["kinds"] == ["dynamic"] and w["matches"] == 1 and w["max_len"] == 3 and w["max_dist"] == 1 and w["out"] == len(PAYLOADS["run4_at_%d" % s][0]), (s, w)
    blob = sim_out["runs"]
    (_, _, pay, n_pay, _, _), = bc.members(blob)
    w = bc.walk(blob[pay:pay + n_pay])
    # 3: none; 4, 5, 258, 259: one; 260 (258 + 1), 261 (258 + 2), 262 (258 + 3): one, one, two; 516 (258 + 257), 517 (2 x 258): two; 520: three
    assert w["matches"] == 0 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 2 + 2 + 3 and w["max_len"] == 258 and w["max_dist"] == 1 and not w["code16"], w
    (_, _, pay, n_pay, _, _), = bc.members(sim_out["fibonacci"])
    assert bc.walk(sim_out["fibonacci"][pay:pay + n_pay])["max_code_len"] <= 15
    (_, _, pay, n_pay, _, _), = bc.members(sim_out["fibonacci_eob"])
    assert bc.walk(sim_out["fibonacci_eob"][pay:pay + n_pay])["max_code_len"] == 15           # the limit acted
    (_, _, pay, n_pay, _, _), = bc.members(sim_out["random"])
    assert sim_out["random"][pay] & 7 == 1          # a final stored block


# ---- the CLI on the host ----------------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, blob):
    p = tmp_path / name
    p.write_bytes(blob)
    return str(p)


def _summary_of(err):
    return b"".join(ln + b"\n" for ln in err.split(b"\n") if ln.startswith((b"total reads:", b"reads >= ")))


def _same_stream(cli, args):        # noqa: F811
    rc, plain, err = run(cli, args)
    rc2, comp, err2 = run(cli, args + ["--bgzf"])
    assert rc == 0 and rc2 == 0 and _summary_of(err) == _summary_of(err2) != b""
    assert comp.endswith(bc.EOF_BLOCK) and gzip.decompress(comp) == plain
    rows = bc.members(comp)
    assert [r[5] for r in rows[:-2]] == [dc.MEMBER] * (len(rows) - 2) and sum(r[5] for r in rows) == len(plain)
    blocks, resume, broken = cornetto_amd.bgzf_scan(comp)
    assert not broken and resume == len(comp)
    return plain


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_writer_equals_the_plain_output(cli, tmp_path, name):        # noqa: F811
    """fails on the parent commit: it has no --bgzf"""
    recs, runs = CASES[name]
    bam = _write(tmp_path, "c.bam", fq.bam(recs, sizes=[700, 333, 1000]))
    for min_len, duplex in runs:
        _same_stream(cli, ["seq", "--accel=no", "-m", str(min_len), "--bam", bam] + (["--duplex"] if duplex else []))


def test_host_writer_seams(cli, tmp_path):        # noqa: F811
    recs, sizes = fq.seam_case()
    bam = _write(tmp_path, "s.bam", fq.bam(recs, sizes=sizes))
    for duplex in (False, True):
        assert len(_same_stream(cli, ["seq", "--accel=no", "-m", "0", "--bam", bam] + (["--duplex"] if duplex else []))) > 0


def test_host_writer_by_the_environment(cli, tmp_path):        # noqa: F811
    """CORNETTO_ACCEL=no takes the same path as --accel=no"""
    bam = _write(tmp_path, "c.bam", fq.bam(CASES["quals"][0]))
    env = dict(os.environ, CORNETTO_ACCEL="no")
    p = subprocess.run([cornetto_amd.CLI_PATH, "seq", "-m", "0", "--bam", bam, "--bgzf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and gzip.decompress(p.stdout) == fq.oracle(fq.raw(CASES["quals"][0]), 0).text and p.stdout.endswith(bc.EOF_BLOCK)


def test_usage_and_help(cli, tmp_path):        # noqa: F811
    fastq = _write(tmp_path, "x.fastq", b"@r\nACGT\n+\n!!!!\n")
    rc, out, err = run(cli, ["seq", "--bgzf", fastq])
    assert rc == 1 and out == b"" and b"--bgzf: only with --bam" in err and err.count(b"ERROR]") == 1
    rc, out, err = run(cli, ["seq", "-h"])
    lines = [ln for ln in out.split(b"\n") if b"--bgzf" in ln]
    assert rc == 0 and len(lines) == 1 and b"(not in the reference)" in lines[0] and out.count(b"(extension)") == 2


@pytest.mark.parametrize("name", ["short_block", "cut_record", "fields_l_seq", "first_error_wins"])
def test_malformed_file_leaves_a_cut_stream(cli, tmp_path, name):        # noqa: F811
    """exit 1 and one ERROR line; the members decode to the text of the records in front of the failing one; no end-of-file block"""
    data, err_want = fq.bad_cases()[name]
    bam = _write(tmp_path, "bad.bam", bc.write(data, [150, 90, 120]))
    rc, plain, err = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", bam])
    rc2, comp, err2 = run(cli, ["seq", "--accel=no", "-m", "0", "--bam", bam, "--bgzf"])
    assert rc == 1 and rc2 == 1 and err2.count(b"ERROR]") == 1 and b"total reads" not in err2
    assert plain == fq.oracle(data).text and len(plain) > 0
    assert not comp.endswith(bc.EOF_BLOCK) and all(r[5] > 0 for r in bc.members(comp))
    assert b"".join(bc.inflate_members(comp)) == plain
