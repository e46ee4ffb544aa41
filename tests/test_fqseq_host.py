"""CPU: `seq --fastq FILE [--bgzf]` on the host path (--accel=no / CORNETTO_ACCEL=no: the sequential reader's loop on FILE, through the small
zlib writer under --bgzf), its usage errors and its help line — the product binary and the sanitized build of the same host C, against
`seq FILE`, the oracle's kseq restatement and the golden outputs.  The device path is tests/test_gpu_fqseq.py's."""
import gzip
import os
import subprocess

import pytest

import bgzf_cases as bc
import cornetto_amd
import fqseq_cases as fc
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

TEXTS = dict({"golden": fc.golden_reads(), "rules_mixed": fc.RULES_MIXED}, **{"rule_" + k: v for k, v in fc.RULES.items()})


def _summary_of(err):
    return b"".join(ln + b"\n" for ln in err.split(b"\n") if ln.startswith((b"total reads:", b"reads >= ")))


def _summary(stats, min_len):
    return ("total reads: %d\t%d bases\t%.2f Gbases\nreads >= %d: %d\t%d bases\t%.2f Gbases\n" % (stats[0], stats[1], stats[1] / 1e9, min_len, stats[2], stats[3], stats[3] / 1e9)).encode()


def _files(tmp_path, name):
    """the text as a plain file, bgzip-compressed (small blocks) and gzip-compressed"""
    text = TEXTS[name]
    out = []
    for ext, blob in ((".fq", text), (".bgz.gz", bc.write(text, [700, 333, 1000])), (".gz", gzip.compress(text))):
        p = tmp_path / (name + ext)
        p.write_bytes(blob)
        out.append(str(p))
    return out


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_accel_no_equals_the_positional_file(cli, tmp_path, name):        # noqa: F811
    """fails on the parent commit: it has no --fastq"""
    for m in (0, 4, 100):
        want_text, want_stats, _ = fc.expected(TEXTS[name], m)
        for f in _files(tmp_path, name):
            rc0, ref, err0 = run(cli, ["seq", "-m", str(m), f])
            rc, out, err = run(cli, ["seq", "--accel=no", "-m", str(m), "--fastq", f])
            assert rc0 == 0 and rc == 0 and out == ref == want_text, (name, m, f)
            assert _summary_of(err) == _summary_of(err0) == _summary(want_stats, m)
            rc, comp, err = run(cli, ["seq", "--accel=no", "--fastq", f, "--bgzf", "-m", str(m)])
            assert rc == 0 and comp.endswith(bc.EOF_BLOCK) and gzip.decompress(comp) == want_text and _summary_of(err) == _summary(want_stats, m)
            assert all(r[5] <= 65280 for r in bc.members(comp)) and comp.count(bc.EOF_BLOCK) >= 1
            blocks, resume, broken = cornetto_amd.bgzf_scan(comp)
            assert not broken and resume == len(comp)


def test_golden_outputs(cli, golden_dir, tmp_path):        # noqa: F811
    """fails on the parent commit: it has no --fastq"""
    reads = os.path.join(golden_dir, "reads.fq")
    for args, exp in ((["-m", "100"], "reads.m100.seq.exp"), ([], "reads.default.seq.exp")):
        rc, out, err = run(cli, ["seq", "--accel=no"] + args + ["--fastq", reads])
        assert rc == 0 and out == open(os.path.join(golden_dir, exp), "rb").read()


def test_by_the_environment(tmp_path):
    """fails on the parent commit: it has no --fastq.  CORNETTO_ACCEL=no takes the same path as --accel=no"""
    env = dict(os.environ, CORNETTO_ACCEL="no")
    for f in _files(tmp_path, "rules_mixed"):
        for m in (0, 4):
            want_text, want_stats, _ = fc.expected(fc.RULES_MIXED, m)
            p = subprocess.run([cornetto_amd.CLI_PATH, "seq", "-m", str(m), "--fastq", f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 0 and p.stdout == want_text and _summary_of(p.stderr) == _summary(want_stats, m)
            p = subprocess.run([cornetto_amd.CLI_PATH, "seq", "-m", str(m), "--fastq", f, "--bgzf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 0 and gzip.decompress(p.stdout) == want_text and p.stdout.endswith(bc.EOF_BLOCK)


def test_usage_errors_and_help(cli, tmp_path):        # noqa: F811
    """fails on the parent commit: it has no --fastq"""
    fq, _, _ = _files(tmp_path, "rule_space")
    bam = str(tmp_path / "x.bam")
    open(bam, "wb").write(bc.EOF_BLOCK)
    for args in (["seq", "--fastq", fq, fq], ["seq", "--fastq", fq, "--bam", bam], ["seq", "--duplex", "--fastq", fq], ["seq", "--accel=no", "--fastq", fq, fq]):
        rc, out, err = run(cli, args)
        assert rc == 1 and out == b"" and err.count(b"ERROR]") == 1 and b"total reads" not in err, args
    rc, out, err = run(cli, ["seq", "--bgzf", fq])          # the positional file keeps its refusal
    assert rc == 1 and out == b"" and b"--bgzf: only with --bam" in err and err.count(b"ERROR]") == 1
    rc, out, err = run(cli, ["seq", "-h"])
    lines = [ln for ln in out.split(b"\n") if b"--fastq" in ln]
    assert rc == 0 and len(lines) == 1 and b"(not in the reference)" in lines[0] and b"--bgzf" not in lines[0] and b"(extension)" not in lines[0]
    rc, out, err = run(cli, ["seq", "--accel=no", "--fastq", str(tmp_path / "missing.fq")])
    assert rc == 1 and out == b"" and err.count(b"ERROR]") == 1


# ---- the kernels' index arithmetic on the CPU, under the host sanitizers -------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.all_cases()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tools/sim/fqseq_sim.cc: fq_frame, fx_size and fx_chunk (csrc/fqrec.hpp, csrc/fqseq.hpp) as the kernels call them, every table in a heap
    block of exactly its size, under AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("fqseq_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cornetto_amd"), "fqseq_sim"])
    exe = os.path.join(ROOT, "cornetto_amd", "fqseq_sim")

    def run_sim(text, min_len, window=None, rng=None):
        p = d / "t.fq"
        p.write_bytes(text)
        args = [exe, "--min-len", str(min_len)] + (["--window", str(window)] if window else []) + (["--range", str(rng)] if rng else []) + [str(p)]
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and len(r.stderr.split()) == 6, r.stderr[-3000:]
        f = [int(x) for x in r.stderr.split()]
        return r.stdout, f[0], bool(f[1]), f[2:]
    return run_sim


def check_sim(got, text, m):
    """the device's part and the sequential reader's part make the whole: text, counts, and plain exactly when no record remains"""
    out, rest, plain, stats = got
    want, rest_of = fc.expected(text, m), fc.expected(text[rest:], m)
    assert out + rest_of[0] == want[0] and [a + b for a, b in zip(stats, rest_of[1])] == want[1] and plain == (rest_of[2] == 0), (rest, plain, stats)


def test_sim_every_case_window_and_range(sim):
    """fails on the parent commit: it has neither header.  The same windows and slabs as on the GPU (tests/test_gpu_fqseq.py)"""
    for name, (text, min_lens) in CASES.items():
        longest = fc.longest_record(text)
        for m in min_lens:
            for window in (longest, 2 * longest + 17, None):
                if window and len(text) > 3000 * window:          # (the 10 000 tiny records: no window of one record here)
                    continue
                for rng in (16, 48, None) if len(text) <= 65536 else (4096, None):
                    check_sim(sim(text, m, window, rng), text, m)


def test_sim_not_plain(sim):
    """fails on the parent commit.  Where the text stops being plain records, and a record that holds a byte 0"""
    stopped = 0
    for text in fc.irregular_texts():
        got = sim(text, 0)
        check_sim(got, text, 0)
        stopped += not got[2]
    assert stopped >= 30
    for text, third in fc.zero_byte_texts():
        got = sim(text, 0, None, 16)
        assert got[1] == third and not got[2] and got[0] == fc.expected(text[:third], 0)[0]
    text = fc.long_read_text()
    got = sim(text, 0, 20000)          # a record larger than the window: the device's part ends in front of it
    assert not got[2] and got[0] == fc.expected(text[:got[1]], 0)[0] and text[got[1]:].startswith(b"@long")
