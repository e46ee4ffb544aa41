"""GPU: the text `seq -m` prints, written on the device from FASTQ text (csrc/fqseq.hip, cornetto_fqseq_*, Accel.fastq_seq) and `seq --fastq`,
against the oracle's kseq restatement (tests/fqseq_cases.py: oracle_bind.fastx_parse + helpers.fmt_seq) with exact equality: the text, the
four counts of the summary lines, the record table, where the device stops and whether the sequential reader has to go on.

Every case runs at three windows — the smallest that holds its longest record, a little over twice that plus 17, and the whole text — and
its text is fetched in slabs of 16, 48 and 4096 bytes and as a whole: all four at the smallest window, the last two at the others; a text
above 64 KiB takes the 16- and 48-byte slabs in its first run only (the rule of test_gpu_bamfq.py::slabs), and where the smallest window
would mean thousands of feeds (the 10 000 tiny records, a window of one record each) that window runs once, with the text fetched whole.
Through BGZF blocks a window has to hold one block more.  The index arithmetic of every case went through tools/sim/fqseq_sim.cc under
the host sanitizers first (tests/test_fqseq_host.py)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases as bc
import cornetto_amd
import fqseq_cases as fc
from cornetto_amd import AccelError, Bgzf, FastqBlockError

pytestmark = pytest.mark.gpu
CASES = fc.all_cases()


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def test_the_tile_is_the_librarys(acc):
    assert acc.L.cornetto_fqseq_tile() == fc.TILE == cornetto_amd.FQSEQ_TILE


def fields(text, recs):
    """(name, comment, seq, qual) byte strings of the device's records"""
    out = []
    for r in recs:
        h, nl, cl, L = int(r["head"]), int(r["name_len"]), int(r["comment_len"]), int(r["len"])
        out.append((text[h + 1:h + 1 + nl], text[h + nl + 2:h + nl + 2 + cl] if cl else b"", text[int(r["seq"]):int(r["seq"]) + L], text[int(r["qual"]):int(r["qual"]) + L]))
    return out


def check(got, text, m, what=None):
    """the device's part and the sequential reader's part make the whole: text, counts and records; plain == 0 exactly when records remain"""
    out, stats, recs, rest, plain = got
    want, rest_of = fc.expected(text, m), fc.expected(text[rest:], m)
    assert out + rest_of[0] == want[0], (what, len(out), rest, next((i for i, (a, b) in enumerate(zip(out, want[0])) if a != b), None))
    assert [a + b for a, b in zip(stats, rest_of[1])] == want[1], (what, stats)
    assert plain == (rest_of[2] == 0), (what, rest, plain)
    assert len(recs) + rest_of[2] == want[2] and fields(text, recs) == [tuple(r) for r in fc.ob.fastx_parse(text)[0][:len(recs)]], what
    assert [int(k) for k in recs["keep"]] == [int(int(n) >= m) for n in recs["len"]]
    return got


def windows(text, extra=0):
    least = fc.longest_record(text) + extra
    return [least, 2 * least + 17, max(1, len(text)) + extra]


def slabs(text, m, first_run):
    return (16, 48, 4096, None) if len(fc.expected(text, m)[0]) <= 65536 or first_run else (65521, 4096, None)


def runs_of(text, m, first_run, extra=0):
    """(window, slab) of every run of a case"""
    out = []
    for i, window in enumerate(windows(text, extra)):
        if i == 0 and len(text) > 2000 * window:
            out.append((window, None))
            continue
        out += [(window, s) for s in (slabs(text, m, first_run) if i == 0 else slabs(text, m, first_run)[-2:])]
    return out


# ---- 1-5: every case, window and slab, from plain bytes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_plain(acc, name):
    text, min_lens = CASES[name]
    for k, m in enumerate(min_lens):
        for window, slab in runs_of(text, m, k == 0):
            got = check(acc.fastq_seq(text, m, window=window, slab=slab), text, m, (name, m, window, slab))
            if not name.startswith("strict"):          # (a strict text may end in a cut-off empty read: the reader's)
                assert got[3] == len(text) and got[4], (name, m, window, slab)
    check(acc.fastq_seq(text, min_lens[0], window=windows(text)[1], feeds=3), text, min_lens[0], (name, "feeds"))       # the tail is carried across feeds


def test_golden_cli_outputs(acc, golden_dir):
    text = fc.golden_reads()
    for m, exp in ((100, "reads.m100.seq.exp"), (30000, "reads.default.seq.exp")):
        want = open(os.path.join(golden_dir, exp), "rb").read()
        assert fc.expected(text, m)[0] == want and acc.fastq_seq(text, m)[0] == want
        p = subprocess.run([cornetto_amd.CLI_PATH, "seq", "--fastq", os.path.join(golden_dir, "reads.fq")] + (["-m", "100"] if m == 100 else []), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and p.stdout == want


# ---- 6: the same from BGZF blocks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_bgzf_in(acc, name):
    text, min_lens = CASES[name]
    bs = fc.block_size(text)
    blob = bc.write(text, [bs] * (len(text) // bs + 1))
    for k, m in enumerate(min_lens):
        plain_feed = acc.fastq_seq(text, m)
        for i, window in enumerate(windows(text, bs)):
            for slab in ((4096, None) if i == 0 else (None,)):
                got = check(acc.fastq_seq(blob, m, window=window, slab=slab, bgzf_in=True), text, m, (name, m, window, slab))
                assert got[0] == plain_feed[0] and got[1] == plain_feed[1] and got[3:] == plain_feed[3:] and got[2].tobytes() == plain_feed[2].tobytes()
    check(acc.fastq_seq(blob, min_lens[0], window=windows(text, bs)[1], feeds=3, bgzf_in=True), text, min_lens[0], (name, "feeds"))


def test_bgzf_block_seams_and_a_change_of_kind(acc):
    text, sizes = fc.bgzf_seam_case()
    blob = bc.write(text, sizes)
    for window in (fc.longest_record(text) + max(sizes + [len(text) - sum(sizes)]), 2 * len(text)):          # (the last block takes the rest)
        for slab in (16, None):
            got = check(acc.fastq_seq(blob, 0, window=window, slab=slab, bgzf_in=True), text, 0, (window, slab))
            assert got[3] == len(text) and got[4]
    # plain bytes, then blocks, then plain bytes again: every border inside a record
    text = CASES["seam_tab"][0]
    a, b = len(text) // 3 + 5, 2 * len(text) // 3 + 11
    parts = [text[:a], Bgzf(bc.write(text[a:b], [1000] * 40)), text[b:]]
    for window in (fc.longest_record(text) + 1000, len(text)):
        got = check(acc.fastq_seq(parts, 0, window=window, slab=4096), text, 0, window)
        assert got[3] == len(text) and got[4]
    got = check(acc.fastq_seq([Bgzf(bc.write(text[:a], [1000] * 40)), text[a:]], 0, feeds=2), text, 0)          # blocks first, then plain bytes
    assert got[3] == len(text) and got[4]


# ---- 7: BGZF output -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "long_read", "tiny", "rules_mixed"])
def test_bgzf_out(acc, name):
    """a get's members are cut every 65280 bytes of ITS range, and a window's text is fetched by its own gets: the bytes are the same for
    every slab that is a multiple of 65280 and every window that holds the whole text; otherwise the inflated text is compared"""
    text, min_lens = CASES[name]
    m = min_lens[0]
    want = fc.expected(text, m)[0]
    chains = {}
    least = fc.longest_record(text)
    for window, slab in ((len(text), 65280), (2 * len(text) + 17, 2 * 65280), (len(text), 3 * 65280), (len(text), None), (len(text), 4096), (2 * least + 17, 65280), (least, None)):
        if len(text) > 2000 * window:
            continue
        out, stats, recs, rest, plain = acc.fastq_seq(text, m, window=window, slab=slab, bgzf_out=True)
        blob = b"".join(out)
        assert plain and rest == len(text) and stats == fc.expected(text, m)[1]
        assert gzip.decompress(blob) == want if blob else want == b""
        rows = bc.members(blob)
        assert all(0 < r[5] <= 65280 for r in rows) and sum(r[5] for r in rows) == len(want)
        blocks, resume, broken = cornetto_amd.bgzf_scan(blob)
        assert not broken and resume == len(blob) and len(blocks) == len(rows)
        if slab and slab % 65280 == 0 and window >= len(text):
            chains[(window, slab)] = blob
    assert len(chains) >= 3 and len(set(chains.values())) == 1


# ---- 8: not plain ---------------------------------------------------------------------------------------------------------------------------------------
def test_irregular_text_stops_where_the_sequential_reader_goes_on(acc):
    stopped = 0
    for it, text in enumerate(fc.irregular_texts()):
        got = check(acc.fastq_seq(text, 0), text, 0, it)
        stopped += not got[4]
        if it % 10 == 0:
            check(acc.fastq_seq(text, 60, slab=48), text, 60, it)
    assert stopped >= 30


def test_a_byte_0_stops_in_front_of_its_record(acc):
    for text, third in fc.zero_byte_texts():
        for window in (None, 70):
            out, stats, recs, rest, plain = acc.fastq_seq(text, 0, window=window)
            assert rest == third and not plain and out == fc.expected(text[:third], 0)[0] and stats == fc.expected(text[:third], 0)[1] and len(recs) == 2
    text, third = fc.zero_byte_texts()[1]
    blob = bc.write(text, [50, 50, 50, 50])
    out, stats, recs, rest, plain = acc.fastq_seq(blob, 0, bgzf_in=True)
    assert rest == third and not plain and out == fc.expected(text[:third], 0)[0]


# ---- 9: a damaged block ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["stream", "crc"])
def test_damaged_block(acc, where):
    text, sizes = fc.four_block_text()
    blob = bytearray(bc.write(text, sizes))
    off, size, pay, n_pay, _, _ = bc.members(bytes(blob))[2]
    blob[pay + n_pay // 2 if where == "stream" else off + size - 8] ^= 0x55
    front = fc.whole_records_in(text, sizes[0] + sizes[1])
    for window, slab, feeds in ((None, None, 1), (fc.longest_record(text) + sizes[0], 48, 1), (None, 16, 4)):
        with pytest.raises(FastqBlockError) as e:
            acc.fastq_seq(bytes(blob), 0, window=window, slab=slab, feeds=feeds, bgzf_in=True)
        assert e.value.block == 2 and e.value.refeed == -6
        assert e.value.text == fc.expected(front, 0)[0] and e.value.stats == fc.expected(front, 0)[1] and e.value.rest == len(front)


# ---- 10: one handle, two files ----------------------------------------------------------------------------------------------------------------------------
JOBS = [("tiny", 2, 70000, 4096, False), ("rule_crlf", 0, 40, 16, False), ("long_read", 1000, 100000, None, True), ("align", fc.ALIGN_MIN_LEN, 500, 48, True)]


def job(acc, name, m, window, slab, bgzf_in):
    text = CASES[name][0]
    data = bc.write(text, [fc.block_size(text)] * 200) if bgzf_in else text
    got = acc.fastq_seq(data, m, window=window + (fc.block_size(text) if bgzf_in else 0), slab=slab, bgzf_in=bgzf_in)
    check(got, text, m, name)
    return got[0], got[1], got[2].tobytes(), got[3], got[4]


def test_one_handle_two_files(acc):
    """two different files one after the other on one handle equal the same files on fresh handles: every table and counter the stage reads is
    written in the same feed"""
    seen = {}
    for order in (JOBS, JOBS[::-1]):
        for j in order:
            assert seen.setdefault(j[0], job(acc, *j)) == job(acc, *j)
    for j in JOBS[:2]:
        fresh = cornetto_amd.Accel(0)
        try:
            assert job(fresh, *j) == seen[j[0]]
        finally:
            fresh.close()


def test_workspaces_filled_with_a_pattern():
    """the kind of check tests/test_gpu_ws_fill.py makes for the other stages: every byte of the handle's workspaces set (the development
    build's hook) between two files"""
    import selftest_bind as st
    dev = cornetto_amd.Accel(0, dev=True)
    try:
        want = {j[0]: job(dev, *j) for j in JOBS}
        for byte in (0xFF, 0xA5, 0x00):
            filled, skipped, pinned = st.ws_fill(dev, byte)
            assert sum(filled.values()) > 0 and {"WS_FQ_CNT", "WS_FQ_NL", "WS_FQ_ENDS"} <= set(filled)
            for j in JOBS[::-1]:
                assert job(dev, *j) == want[j[0]], (byte, j[0])
    finally:
        dev.close()


# ---- 11: a record larger than the window ----------------------------------------------------------------------------------------------------------------
def test_record_larger_than_the_window(acc):
    text = fc.long_read_text()
    for data, bgzf_in in ((text, False), (bc.write(text, [60000] * 4), True)):
        with pytest.raises(AccelError) as e:
            acc.fastq_seq(data, 0, window=70000, bgzf_in=bgzf_in)
        assert e.value.status == -4 and e.value.taken == 0


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


def run(cli, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return p.returncode, p.stdout, p.stderr


def summary_of(err):
    return [ln for ln in err.decode(errors="replace").splitlines() if ln.startswith(("total reads:", "reads >= "))]


def cli_text():
    """several windows of every kind of record: the seam records, the long read, the rules (CRLF, comments, an empty read)"""
    return CASES["seam_tab"][0] + fc.long_read_text() + b"".join(v for k, v in fc.RULES.items() if k != "no_last_newline") + CASES["align"][0] + fc.RULES["no_last_newline"]


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_cli_equals_the_positional_file(cli, tmp_path, kind):
    text = cli_text()
    p = tmp_path / ("reads.fq" + ("" if kind == "plain" else ".gz"))
    p.write_bytes(text if kind == "plain" else bc.write(text, [20000] * 20) if kind == "bgzf" else gzip.compress(text))
    envs = [{}, {"CORNETTO_BGZF": "0"}, {"CORNETTO_FASTQ_PIECE": "30000", "CORNETTO_EMIT_SLAB": "4099"},
            {"CORNETTO_FASTQ_WINDOW": "110000", "CORNETTO_EMIT_SLAB": "65280", "CORNETTO_CLI_TRACE": "1"}]
    for m, env in zip((0, 60, 30000, 0), envs):
        want = run(cli, ["seq", "-m", str(m), str(p)])
        assert want[0] == 0 and want[1] == fc.expected(text, m)[0] and len(summary_of(want[2])) == 2
        got = run(cli, ["seq", "-m", str(m), "--fastq", str(p)], env)
        assert got[0] == 0 and got[1] == want[1] and summary_of(got[2]) == summary_of(want[2]) and b"WARNING" not in got[2], (kind, m, env, got[2][-1500:])
        z = run(cli, ["seq", "-m", str(m), "--fastq", str(p), "--bgzf"], env)
        assert z[0] == 0 and z[1].endswith(bc.EOF_BLOCK) and z[1].count(bc.EOF_BLOCK) == 1 and gzip.decompress(z[1]) == want[1] and summary_of(z[2]) == summary_of(want[2])
    assert b"[cli trace] seq --fastq: feed" in got[2]


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_cli_small_pieces_and_slabs(cli, tmp_path, kind):
    """CORNETTO_FASTQ_PIECE=1500 CORNETTO_EMIT_SLAB=16: a record in several pieces, its text in many slabs"""
    text = fc.golden_reads() + fc.RULES_MIXED
    p = tmp_path / ("small.fq" + ("" if kind == "plain" else ".gz"))
    p.write_bytes(text if kind == "plain" else bc.write(text, [1000] * 20) if kind == "bgzf" else gzip.compress(text))
    env = {"CORNETTO_FASTQ_PIECE": "1500", "CORNETTO_EMIT_SLAB": "16", "CORNETTO_FASTQ_WINDOW": "2000"}
    for m in (0, 100):
        want = run(cli, ["seq", "-m", str(m), str(p)])
        got = run(cli, ["seq", "-m", str(m), "--fastq", str(p)], env)
        assert want[0] == 0 and got[0] == 0 and got[1] == want[1] == fc.expected(text, m)[0] and summary_of(got[2]) == summary_of(want[2]), (kind, m, got[2][-1500:])
        z = run(cli, ["seq", "-m", str(m), "--fastq", str(p), "--bgzf"], env)
        assert z[0] == 0 and z[1].endswith(bc.EOF_BLOCK) and gzip.decompress(z[1]) == want[1] and summary_of(z[2]) == summary_of(want[2])


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_cli_a_file_that_turns_irregular_half_way(cli, tmp_path, kind):
    irregular = max(fc.irregular_texts(), key=len)
    assert fc.expected(irregular, 0)[2] > 5
    text = fc.golden_reads() + irregular + fc.golden_reads()
    p = tmp_path / ("half." + kind)
    p.write_bytes(text if kind == "plain" else bc.write(text, [5000] * 100) if kind == "bgzf" else gzip.compress(text))
    for m, env in ((0, {}), (100, {"CORNETTO_FASTQ_PIECE": "1500", "CORNETTO_EMIT_SLAB": "4099", "CORNETTO_FASTQ_WINDOW": "9000"})):
        want = run(cli, ["seq", "-m", str(m), str(p)])
        got = run(cli, ["seq", "-m", str(m), "--fastq", str(p)], env)
        assert got[0] == 0 and got[1] == want[1] and summary_of(got[2]) == summary_of(want[2]) and len(summary_of(got[2])) == 2, (kind, m, env, got[2][-1500:])
        z = run(cli, ["seq", "-m", str(m), "--fastq", str(p), "--bgzf"], env)
        assert z[0] == 0 and z[1].endswith(bc.EOF_BLOCK) and gzip.decompress(z[1]) == want[1] and summary_of(z[2]) == summary_of(want[2])


def test_cli_record_larger_than_the_window(cli, tmp_path):
    text = fc.long_read_text()
    for kind, blob in (("plain", text), ("bgzf", bc.write(text, [60000] * 4))):
        p = tmp_path / ("long." + kind)
        p.write_bytes(blob)
        want = run(cli, ["seq", "-m", "0", str(p)])
        a, b = run(cli, ["seq", "-m", "0", "--fastq", str(p)]), run(cli, ["seq", "-m", "0", "--fastq", str(p)], {"CORNETTO_FASTQ_WINDOW": "70000"})
        assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == want[1] == fc.expected(text, 0)[0]
        assert summary_of(a[2]) == summary_of(b[2]) == summary_of(want[2])
        assert b"WARNING" in b[2] and b"on the host" in b[2] and b"WARNING" not in a[2]
    for bad in ("0", "12x", str(1 << 32)):
        got = run(cli, ["seq", "--fastq", str(p)], {"CORNETTO_FASTQ_WINDOW": bad})
        assert got[0] == 1 and got[1] == b"" and got[2].count(b"ERROR]") == 1


@pytest.mark.parametrize("where", ["stream", "crc", "not_a_block", "cut"])
def test_cli_damaged_block(cli, tmp_path, where):
    text, sizes = fc.four_block_text()
    blob = bytearray(bc.write(text, sizes))
    off, size, pay, n_pay, _, _ = bc.members(bytes(blob))[2]
    if where in ("stream", "crc"):
        blob[pay + n_pay // 2 if where == "stream" else off + size - 8] ^= 0x55
    elif where == "not_a_block":
        blob[off + 12] ^= 0xFF          # no BC subfield: the chain breaks in front of block 2
    else:
        blob = blob[:off + size // 2]   # the file ends inside block 2
    p = tmp_path / "bad.fq.gz"
    p.write_bytes(bytes(blob))
    front = fc.expected(fc.whole_records_in(text, sizes[0] + sizes[1]), 0)[0]
    for env in ({}, {"CORNETTO_FASTQ_WINDOW": "1500", "CORNETTO_EMIT_SLAB": "48"}):
        got = run(cli, ["seq", "-m", "0", "--fastq", str(p)], env)
        assert got[0] == 1 and got[1] == front and got[2].count(b"ERROR]") == 1 and b"block 2" in got[2] and not summary_of(got[2]), (where, env, got[2][-1500:])
        z = run(cli, ["seq", "-m", "0", "--fastq", str(p), "--bgzf"], env)
        assert z[0] == 1 and z[2].count(b"ERROR]") == 1 and not summary_of(z[2]) and not z[1].endswith(bc.EOF_BLOCK)
        assert b"".join(bc.inflate_members(z[1])) == front
