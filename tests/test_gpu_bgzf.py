"""GPU: BGZF-compressed text inflated on the device — cornetto_text_inflate (bgzf_inflate, bgzf_crc32) against zlib over every deflate shape
of tests/bgzf_cases.py, a multi-block FASTA text whose seams fall on '>' , names and newlines, bad blocks as data (their mutations went
through the sanitizer program of tests/test_bgzf_host.py first), and the CLI's fourth source stream_bgzf_fasta() with its fallbacks."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases as bc
import cornetto_amd
import fixasm_cases as fc
import oracle_bind as ob
from helpers import golden, tricky_fastx

pytestmark = pytest.mark.gpu

CASES = bc.cases()


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


# ---- 1. every deflate shape ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_inflates_to_zlibs_bytes(acc, name):
    data, kw, check = CASES[name]
    m = bc.member(data, **kw)
    pay = bc.members(m)[0]
    assert check(bc.walk(m[pay[2]:pay[2] + pay[3]])), name
    other = bc.member(b">seam\nACGTTTAGGG\n", level=1)
    for blob in (m + bc.EOF_BLOCK, m + bc.EOF_BLOCK + other + m + bc.EOF_BLOCK):
        got, first_bad = acc.bgzf_inflate(blob)
        exp = bc.inflate_members(blob)
        assert first_bad == -1 and acc.last_status == 0
        assert exp[0] == data and got == b"".join(exp)
    names = [n for n, _ in acc.inflate_timing]
    assert "bgzf_inflate" in names and "bgzf_crc32" in names


# ---- 2. a multi-block FASTA text ----------------------------------------------------------------------------------------------------------
def fasta_from_tricky(seed, n_rec):
    """the records of helpers.tricky_fastx(strict=True) written as FASTA: their names and comments (tabs, double spaces), wrapped at
    several widths, CRLF and empty lines among them, lower case and N in the bases"""
    rng = np.random.default_rng(seed)
    recs, rc = ob.fastx_parse(tricky_fastx(rng, n_rec, strict=True))
    out = []
    for i, (name, comment, seq, _) in enumerate(recs):
        eol = b"\r\n" if i % 7 == 3 else b"\n"
        seq = seq.replace(b"\r", b"")          # (kseq reads the "\r" of an empty CRLF read as a base; as a FASTA line of its own it is not plain)
        comment = (comment or b"").replace(b"\r", b"")
        out.append(b">" + name + (b" " + comment if comment else b"") + eol)
        w = [60, 80, 7, 100000][i % 4]
        for k in range(0, len(seq), w):
            out.append(seq[k:k + w] + eol)
            if i % 11 == 5 and eol == b"\n":
                out.append(eol)
    return b"".join(out)


def seam_kinds(text, sizes):
    """what the first byte of every block but the first is: '>' , a byte of a header line, a newline, or a base"""
    kinds, at = set(), 0
    for n in sizes[:-1]:
        at += n
        if at >= len(text):
            break
        line = text.rfind(b"\n", 0, at) + 1
        kinds.add(">" if text[at:at + 1] == b">" else "newline" if text[at:at + 1] in (b"\n", b"\r") else "name" if text[line:line + 1] == b">" else "base")
    return kinds


def test_multi_block_fasta_equals_the_plain_text(acc):
    text = fasta_from_tricky(41, 1500)
    assert 250_000 < len(text) < 400_000 and b"\r\n" in text and b"\n\n" in text and any(c in text for c in (b"a", b"c", b"g", b"t"))
    rng = np.random.default_rng(8)
    sizes, left = [], len(text)
    while left > 0:
        n = min(left, int(np.exp(rng.uniform(0.0, np.log(65280.0)))))      # 1 .. 65280, small blocks as likely as large ones
        sizes.append(max(1, n))
        left -= sizes[-1]
    k = int(np.argmax(sizes))                       # the largest block is cut in two at its last '>': one seam is sure to sit there
    cut = text.rfind(b">", 0, sum(sizes[:k + 1])) - sum(sizes[:k])
    sizes[k:k + 1] = [cut, sizes[k] - cut]
    assert min(sizes) == 1 and max(sizes) > 30000 and sum(sizes) == len(text)
    assert {">", "name", "newline"} <= seam_kinds(text, sizes), seam_kinds(text, sizes)
    blob = bc.write(text, sizes=sizes)
    a = acc.fasta_split(text, final=True, want_seqs=True)
    b = acc.fasta_split_bgzf(blob, final=True, want_seqs=True, want_names=True)
    assert len(a[0]) > 1000 and np.array_equal(a[0], b[0]) and a[1:3] == b[1:3]
    assert b[4] == [text[int(r["head"]) + 1:int(r["head"]) + 1 + int(r["name_len"])] for r in a[0]]
    assert np.array_equal(acc.sdust(a[3], 20, 64), acc.sdust(b[3], 20, 64))
    assert np.array_equal(acc.telofind(a[3], b"TTAGGG"), acc.telofind(b[3], b"TTAGGG"))
    a[3].close()
    b[3].close()
    got, first_bad = acc.bgzf_inflate(blob)
    assert got == text and first_bad == -1


# ---- 3. bad blocks are data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_a_bad_block_is_reported_and_the_others_keep_their_bytes(acc, k):
    """block 3 of six: footer CRC flipped, ISIZE one lower, ISIZE one higher, a payload byte zeroed, n_src shortened by 4.  The blocks are
    laid out with 64 bytes of canary between them: a bad block writes inside its own range at most"""
    blob, cut = bc.bad_block_files()[k]
    blocks, resume, broken = cornetto_amd.bgzf_scan(blob)
    assert len(blocks) == 6 and resume == len(blob) and not broken
    blocks["n_src"][3] += cut
    blocks["dst"] += 64 * np.arange(1, 7)
    got, first_bad = acc.bgzf_inflate(blob, blocks=blocks, fill=0xA5)
    assert first_bad == 3 and acc.last_status == -6
    _, good = bc.six_blocks()
    exp = bc.inflate_members(good)
    free = np.ones(len(got), dtype=bool)
    for i, b in enumerate(blocks):
        d, n = int(b["dst"]), int(b["n_dst"])
        free[d:d + n] = False
        if i != 3:
            assert got[d:d + n] == exp[i], i
    assert free.sum() >= 64 * 6 + 256 and bytes(np.frombuffer(got, dtype=np.uint8)[free]) == b"\xa5" * int(free.sum())


# ---- 4. the CLI ---------------------------------------------------------------------------------------------------------------------------
def run(args, cwd, env=None):
    e = dict(os.environ)
    for k in ("CORNETTO_ACCEL", "CORNETTO_BGZF", "CORNETTO_CLI_WHOLE", "CORNETTO_FASTQ_PIECE", "CORNETTO_CLI_TRACE"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([cornetto_amd.CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=cwd)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def dirs(golden_dir, tmp_path_factory):
    """the same file names in two directories: plain/ holds the FASTA files, bgzf/ the same text as BGZF (stdout that names its input is equal)"""
    plain, bz = tmp_path_factory.mktemp("plain"), tmp_path_factory.mktemp("bgzf")
    texts = {"mix.fa": gzip.open(os.path.join(golden_dir, "mix.fa.gz")).read(), "probe.fa": open(os.path.join(golden_dir, "probe.fa"), "rb").read()}
    rng = np.random.default_rng(9)
    for name, text in texts.items():
        (plain / name).write_bytes(text)
        (bz / name).write_bytes(bc.write(text, sizes=[int(x) for x in rng.integers(1, 65281, size=4)]))
    for d in (plain, bz):
        (d / "mix.paf").write_text(fc.MIX_PAF)
    return str(plain), str(bz)


CLI_CASES = [(["sdust"], "sdust"), (["telofind"], "telofind"), (["telostats", "-b", "out.bed"], None), (["nx"], None), (["report"], None), (["fixasm"], None)]


@pytest.mark.parametrize("fa", ["mix.fa", "probe.fa"])
@pytest.mark.parametrize("args,gold", CLI_CASES)
def test_cli_on_bgzf_prints_what_the_plain_file_prints(dirs, golden_dir, args, gold, fa):
    plain, bz = dirs
    a = args + [fa] + (["mix.paf"] if args[0] == "fixasm" else [])
    want = run(a, plain)
    got = run(a, bz, {"CORNETTO_CLI_TRACE": "1"})
    off = run(a, bz, {"CORNETTO_CLI_TRACE": "1", "CORNETTO_BGZF": "0"})
    assert got[:2] == want[:2] and off[:2] == want[:2], (got[0], want[0], got[2][-2000:])
    assert want[0] == 0
    if gold:
        assert got[1] == golden(golden_dir, fa[:-3] + "." + gold + ".exp")
    assert b"text inflated on the device" in got[2] and b"block chain walked" in got[2] and b"bgzf: fallback" not in got[2]
    assert b"text inflated on the device" not in off[2] and b"bgzf:" not in off[2]
    if args[0] == "telostats":
        assert open(os.path.join(plain, "out.bed"), "rb").read() == open(os.path.join(bz, "out.bed"), "rb").read()


# ---- 5. fallbacks -------------------------------------------------------------------------------------------------------------------------
def _fallback_files(golden_dir):
    text = gzip.open(os.path.join(golden_dir, "mix.fa.gz")).read()
    text = text[text.find(b">", 900_000):]             # its last eight records, 166 kB
    good = bc.write(text, sizes=[30000, 50000, 20000])
    corrupt = bytearray(good)
    off, size, pay, n_pay, _, _ = bc.members(good)[1]
    corrupt[pay + n_pay // 2] ^= 0x10
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGTTTAGGG" * (i % 9 + 1), b"I" * (10 * (i % 9 + 1))) for i in range(300))
    half = text[:text.find(b">", 5000)]
    return {
        "plain_gzip": (open(os.path.join(golden_dir, "mix.fa.gz"), "rb").read(), False),
        "gzip_member_appended": (good + gzip.compress(b">tail\nACGTACGT\n"), False),
        "corrupt_block": (bytes(corrupt), False),
        "bgzf_fastq": (bc.write(fq, sizes=[5000]), False),
        "fasta_then_fastq": (bc.write(half + fq + text[len(half):], sizes=[40000, 65000]), True),
    }


@pytest.mark.parametrize("which", ["plain_gzip", "gzip_member_appended", "corrupt_block", "bgzf_fastq", "fasta_then_fastq"])
@pytest.mark.parametrize("sub", ["sdust", "telofind"])
def test_cli_falls_back_with_the_same_output(golden_dir, tmp_path, which, sub):
    blob, device_first = _fallback_files(golden_dir)[which]
    (tmp_path / "in.fa.gz").write_bytes(blob)
    got = run([sub, "in.fa.gz"], str(tmp_path), {"CORNETTO_CLI_TRACE": "1"})
    off = run([sub, "in.fa.gz"], str(tmp_path), {"CORNETTO_CLI_TRACE": "1", "CORNETTO_BGZF": "0"})
    assert got[:2] == off[:2], (got[0], off[0], got[2][-2000:], off[2][-2000:])
    assert b"bgzf: fallback (" in got[2] and b"bgzf:" not in off[2]
    assert (b"text inflated on the device" in got[2]) == device_first
    if which != "corrupt_block":
        assert got[0] == 0 and len(got[1]) > 0
