"""CPU: the host side of the BGZF path — the test material keeps the shapes it is there for, cornetto_bgzf_scan() walks a chain whatever the
cuts of the buffer, and the device's deflate decoder (csrc/inflate.hpp) run on the CPU under AddressSanitizer + UBSan against zlib
(tools/sim/inflate_sim.cc: a stand-alone program) over every case, their mutations, truncations and wrong sizes: the argument for the
kernels' bounds.  The host path of the CLI (CORNETTO_ACCEL=no) reads a BGZF file as it always did."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_cases as bc
import cornetto_amd
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_keeps_its_shape(name):
    data, kw, check = CASES[name]
    blob = bc.member(data, **kw)
    (off, size, pay, n_pay, crc, isize), = bc.members(blob)
    w = bc.walk(blob[pay:pay + n_pay])
    assert w["out"] == len(data) == isize and check(w), (name, w)
    if name == "random_stored":
        assert size == 65316
    if name == "empty":
        assert blob == bc.EOF_BLOCK and len(blob) == 28


def _small_file():
    parts = [b">a x\nACGT\n", b"", b">b\nAC\r\nGT\n" * 3, b"N" * 70, b">c\n"]
    blob = b"".join(bc.member(p, level=[0, 6, 9, 1, 6][i], strategy=[0, 4, 0, 0, 0][i]) for i, p in enumerate(parts))
    return blob + bc.member(b"TTAGGG" * 20, extra_front=b"XY\x03\x00abc") + bc.EOF_BLOCK


def _expect(blob, upto=None):
    rows, dst = [], 0
    for off, size, pay, n_pay, crc, isize in bc.members(blob):
        if upto is not None and off + size > upto:
            break
        rows.append((pay, dst, n_pay, isize, crc, 0))
        dst += isize
    return np.array(rows, dtype=cornetto_amd.BGZF_DT)


def test_scan_whatever_the_cut():
    """the file handed over in two pieces cut at EVERY offset: a header, an extra field or a footer split by the cut is carried over through
    the resume offset, and the blocks are those of the independent walker of the tests"""
    blob = _small_file()
    exp = _expect(blob)
    assert len(exp) == 7
    whole, resume, broken = cornetto_amd.bgzf_scan(blob)
    assert np.array_equal(whole, exp) and resume == len(blob) and not broken
    for cut in range(len(blob) + 1):
        a, r1, br1 = cornetto_amd.bgzf_scan(blob[:cut])
        assert not br1 and np.array_equal(a, _expect(blob, cut)), cut
        assert r1 == (int(a["src"][-1] + a["n_src"][-1]) + 8 if len(a) else 0), cut
        b, r2, br2 = cornetto_amd.bgzf_scan(blob[r1:], file_off=r1, dst=int(a["n_dst"].sum()))
        assert not br2 and r2 == len(blob) and np.array_equal(np.concatenate([a, b]), exp), cut


def test_scan_extra_subfield_in_front_of_bc():
    blob = bc.member(b">x\nACGT\n", extra_front=b"RA\x04\x00wxyz" + b"Q1\x00\x00")
    b, resume, broken = cornetto_amd.bgzf_scan(blob)
    assert len(b) == 1 and resume == len(blob) and not broken
    assert int(b["src"][0]) == 12 + 8 + 4 + 6 and int(b["n_dst"][0]) == 8


def test_scan_broken_chains():
    good = bc.write(b">x\n" + bc.acgt(1000, 1) + b"\n", sizes=[300, 300])
    n = len(bc.members(good))
    for tail, is_broken in ((gzip.compress(b">y\nAC\n"), True), (b"xx", True), (b"\x1f\x8b\x08\x00", True), (good[:11], False), (b"\x1f", False)):
        b, resume, broken = cornetto_amd.bgzf_scan(good + tail)
        assert len(b) == n and resume == len(good) and broken == is_broken, tail
    # a member whose BC subfield is missing, has another size, or whose ISIZE is above 64 KiB is not BGZF
    m = bytearray(bc.member(b"ACGT"))
    for at, v in ((12, ord("X")), (14, 3), (len(m) - 2, 2)):
        bad = bytearray(m)
        bad[at] = v
        assert cornetto_amd.bgzf_scan(bytes(bad))[1:] == (0, True), at
    assert cornetto_amd.bgzf_scan(b"")[1:] == (0, False)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_sim")
    exe = str(d / "inflate_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "sim", "inflate_sim.cc"), "-lz", "-o", exe])
    return exe, d


def _run_sim(exe, files, n_mut):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, "--mut", str(n_mut), "--seed", "7"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "FAIL" not in err, (p.returncode, p.stdout, err[-3000:])
    words = p.stdout.decode().split()
    return int(words[1]), int(words[3]), int(words[5].lstrip("("))      # members, trials, trials good for zlib


def test_decoder_under_the_sanitizers_against_zlib(sim):
    """every case as a file of its own (the case's member and the empty block), each member as it is, with 200 seeded single-bit and
    single-byte changes of its deflate stream (half of them in its first 64 bytes), with n_src cut short and n_dst off by one: where
    zlib's raw inflate gives exactly n_dst bytes with the footer's CRC the decoder gives the same bytes, everywhere else it reports the
    block bad; no sanitizer report, exit 0"""
    exe, d = sim
    files = []
    for name, (data, kw, _) in sorted(CASES.items()):
        f = d / (name + ".gz")
        f.write_bytes(bc.member(data, **kw) + bc.EOF_BLOCK)
        files.append(str(f))
    members, trials, good = _run_sim(exe, files, 200)
    assert members == 2 * len(CASES)
    assert trials - members * 10 >= 2000 and good >= members       # (at most 10 trials of a member are not mutations)


def test_decoder_on_the_bad_blocks_of_the_device_test(sim):
    """the changes tests/test_gpu_bgzf.py makes to block 3 of its six-block file go through the sanitizer program first: the four changed
    files here (n_src - 4, the fifth, is one of the program's trials of every member)"""
    exe, d = sim
    files = []
    for k, (blob, cut) in enumerate(bc.bad_block_files()):
        if cut == 0:
            (d / ("bad%d.gz" % k)).write_bytes(blob)
            files.append(str(d / ("bad%d.gz" % k)))
    assert len(files) == 4
    _run_sim(exe, files, 50)


@pytest.mark.parametrize("args,exp", [(["telofind"], "mix.telofind.exp"), (["sdust"], "mix.sdust.exp"), (["sdust", "-w", "32", "-t", "10"], "mix.w32t10.sdust.exp")])
def test_host_path_reads_bgzf_as_before(golden_dir, tmp_path, args, exp):
    """CORNETTO_ACCEL=no: gzread() inflates a BGZF file like any gzip file; the goldens are printed"""
    text = gzip.open(os.path.join(golden_dir, "mix.fa.gz")).read()
    f = tmp_path / "mix.bgzf.fa.gz"
    f.write_bytes(bc.write(text))
    env = dict(os.environ, CORNETTO_ACCEL="no", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CORNETTO_CLI_TRACE="1")
    p = subprocess.run([cornetto_amd.CLI_PATH] + args + [str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and p.stdout == golden(golden_dir, exp)
    assert b"bgzf:" not in p.stderr


def test_struct_layout():
    assert cornetto_amd.BGZF_DT.itemsize == 32 == struct.calcsize("<qqiiIi")
