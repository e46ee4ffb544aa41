"""GPU: BGZF members made on the device (csrc/deflate.hip, cornetto_text_deflate) and `seq --bam --bgzf`, with zlib as the reference: every
member of every payload of tests/deflate_cases.py inflates to its piece with the right CRC-32 and ISIZE, the size conditions hold, the
bytes are those of the same encoder run on the CPU (tools/sim/deflate_sim.cc, built here without sanitizers) and do not depend on what
the handle did before; the CLI's stream gunzips to what the same command prints without --bgzf, whatever the slab and the window.
Every payload went through the sanitized build of the CPU program first (tests/test_deflate_host.py).  Bad input here is a bad BAM, which
the command refuses with a status."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

import bamfq_cases as fq
import bgzf_cases as bc
import cornetto_amd
import deflate_cases as dc
from cornetto_amd import AccelError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOADS = dc.payloads()
CASES = fq.valid_cases()


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def device_out(acc):
    """{name: the chain of the payload}, each made once"""
    return {name: acc.bgzf_deflate(data, at=at) for name, (data, at) in PAYLOADS.items()}


@pytest.fixture(scope="module")
def sim_out(tmp_path_factory):
    """the same encoder on the CPU, the 64 lanes one after the other: {name: chain}"""
    d = tmp_path_factory.mktemp("deflate_sim")
    exe = str(d / "deflate_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "sim", "deflate_sim.cc"), "-lz", "-o", exe])
    files = []
    for name, (data, at) in sorted(PAYLOADS.items()):
        (d / name).write_bytes(data[at:])
        files.append(str(d / name))
    subprocess.check_call([exe] + files, stdout=subprocess.DEVNULL)
    return {name: (d / (name + ".bgzf")).read_bytes() for name in PAYLOADS}


@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_members_against_zlib(acc, device_out, sim_out, name):
    data, at = PAYLOADS[name]
    payload, blob = data[at:], device_out[name]
    sizes = dc.check_chain(blob, payload)              # zlib's bytes, CRC-32, ISIZE, a member every 65280 bytes, at most 65311 bytes each
    dc.check_sizes(name, sizes, payload)
    assert gzip.decompress(blob + bc.EOF_BLOCK) == payload
    assert blob == sim_out[name], next((i for i, (a, b) in enumerate(zip(blob, sim_out[name])) if a != b), (len(blob), len(sim_out[name])))
    assert acc.bgzf_deflate(data, at=at) == blob and acc.deflate_members == len(sizes)       # the second call gives the same bytes
    if blob:
        text, bad = acc.bgzf_inflate(blob)              # the project's own decoder takes it
        assert bad == -1 and text == payload


def test_nothing_is_left_over(acc, device_out):
    """one handle compresses the random payload (a stored member fills its staging), then a short payload of runs into the same
    workspaces: the bytes of a fresh handle"""
    a = cornetto_amd.Accel(0)
    try:
        first = a.bgzf_deflate(PAYLOADS["random"][0])
        then = a.bgzf_deflate(PAYLOADS["runs"][0])
    finally:
        a.close()
    b = cornetto_amd.Accel(0)
    try:
        fresh = b.bgzf_deflate(PAYLOADS["runs"][0])
    finally:
        b.close()
    assert first == device_out["random"] and then == fresh == device_out["runs"]


def test_a_part_of_the_text(acc):
    """n bytes from an offset: the members of exactly that range"""
    data, at = PAYLOADS["odd_offset"]
    blob = acc.bgzf_deflate(data, at=at + 3, n=dc.MEMBER + 77)
    dc.check_chain(blob, data[at + 3:at + 3 + dc.MEMBER + 77])
    assert acc.bgzf_deflate(data, at=5, n=0) == b"" and acc.deflate_members == 0


def test_output_too_small_is_refused(acc):
    """room for ceil(n / 65280) * 65536 bytes or CORNETTO_E_ARG, and nothing is written"""
    data = PAYLOADS["len_65281"][0]
    for cap in (65536, 2 * 65536 - 1):
        text, out = acc._text_from(data), acc._text_from(b"\x5a" * cap)
        try:
            n_out, members = C.c_int64(-1), C.c_int64(-1)
            rc = acc.L.cornetto_text_deflate(acc.h, text, 0, len(data), out, 0, C.byref(n_out), C.byref(members))
            assert rc == -3 and b"room for 131072" in acc.L.cornetto_accel_last_error(acc.h)
            assert acc._text_bytes(out, cap) == b"\x5a" * cap
            rc = acc.L.cornetto_text_deflate(acc.h, text, 0, len(data), out, 1, C.byref(n_out), C.byref(members)) if cap > 65536 else -3
            assert rc == -3
        finally:
            acc.L.cornetto_text_free(acc.h, text)
            acc.L.cornetto_text_free(acc.h, out)
    with pytest.raises(AccelError):
        acc.bgzf_deflate(data, out_cap=2 * 65536 - 1)
    assert len(acc.bgzf_deflate(data, out_cap=2 * 65536)) > 0


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------
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


def same_stream(cli, args, env=None, want=None):
    """--bgzf: a BGZF file with the end-of-file block whose content is what the command prints without the option -> (members, text)"""
    if want is None:
        want = run(cli, args, env)
    got = run(cli, args + ["--bgzf"], env)
    assert want[0] == 0 and got[0] == 0 and lines_of(got[2]) == lines_of(want[2]), got[2][-1500:]
    assert got[1].endswith(bc.EOF_BLOCK) and gzip.decompress(got[1]) == want[1]
    rows = bc.members(got[1])
    assert all(r[1] <= dc.MAX_SIZE and r[5] <= dc.MEMBER for r in rows) and b"".join(bc.inflate_members(got[1])) == want[1]
    blocks, resume, broken = cornetto_amd.bgzf_scan(got[1])
    assert not broken and resume == len(got[1])
    return rows, want


@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_stream_equals_the_plain_output(cli, tmp_path, name):
    """fails on the parent commit: it has no --bgzf"""
    recs, runs = CASES[name]
    p = tmp_path / (name + ".bam")
    p.write_bytes(fq.bam(recs, sizes=[5000] * 400))
    for min_len, duplex in runs:
        args = ["seq", "-m", str(min_len), "--bam", str(p)] + (["--duplex"] if duplex else [])
        rows, want = same_stream(cli, args)
        assert want[1] == fq.oracle(fq.raw(recs), min_len, duplex).text
        # one slab: a member every 65280 bytes of the text, the last one shorter, then the end-of-file block
        assert [r[5] for r in rows] == [dc.MEMBER] * (len(want[1]) // dc.MEMBER) + ([len(want[1]) % dc.MEMBER] if len(want[1]) % dc.MEMBER else []) + [0]


def test_cli_seams(cli, tmp_path):
    recs, sizes = fq.seam_case()
    p = tmp_path / "s.bam"
    p.write_bytes(fq.bam(recs, sizes=sizes))
    for duplex in (False, True):
        rows, want = same_stream(cli, ["seq", "-m", "0", "--bam", str(p)] + (["--duplex"] if duplex else []))
        assert len(want[1]) > 0


@pytest.mark.parametrize("env", [{"CORNETTO_EMIT_SLAB": "1000"}, {"CORNETTO_EMIT_SLAB": "65280"}, {"CORNETTO_EMIT_SLAB": "65281"},
                                 {"CORNETTO_BAM_WINDOW": "70000"}, {"CORNETTO_BAM_WINDOW": "70000", "CORNETTO_EMIT_SLAB": "4099"}],
                         ids=lambda e: ",".join("%s=%s" % (k[9:], v) for k, v in sorted(e.items())))
def test_cli_slabs_and_windows_cut_blocks_not_content(cli, tmp_path, env):
    """where the members are cut depends on the slab and the window; the content never does"""
    recs, _ = CASES["many_small"]
    p = tmp_path / "m.bam"
    p.write_bytes(fq.bam(recs, sizes=[5000] * 400))
    args = ["seq", "-m", "0", "--bam", str(p)]
    plain = run(cli, args)
    assert len(plain[1]) > 3 * dc.MEMBER
    rows, _ = same_stream(cli, args, env, want=plain)
    slab = int(env.get("CORNETTO_EMIT_SLAB", 1 << 30))
    assert max(r[5] for r in rows) <= min(slab, dc.MEMBER)
    if "CORNETTO_BAM_WINDOW" not in env:             # one window: its text slab by slab, a slab member by member
        n, want_sizes = len(plain[1]), []
        for at in range(0, n, slab):
            m = min(slab, n - at)
            want_sizes += [dc.MEMBER] * (m // dc.MEMBER) + ([m % dc.MEMBER] if m % dc.MEMBER else [])
        assert [r[5] for r in rows] == want_sizes + [0]


def test_cli_record_larger_than_the_window(cli, tmp_path):
    """device members, the WARNING, host members: one valid stream"""
    recs = CASES["one_long"][0]
    p = tmp_path / "long.bam"
    p.write_bytes(fq.bam(recs, sizes=[60000] * 40))
    args = ["seq", "-m", "0", "--bam", str(p)]
    plain = run(cli, args)
    assert plain[0] == 0 and plain[1] == fq.oracle(fq.raw(recs), 0).text
    got = run(cli, args + ["--bgzf"], {"CORNETTO_BAM_WINDOW": "200000"})
    assert got[0] == 0 and b"on the host" in got[2] and lines_of(got[2])[-2:] == lines_of(plain[2])
    assert got[1].endswith(bc.EOF_BLOCK) and gzip.decompress(got[1]) == plain[1]
    assert len(bc.members(got[1])) > 3 and not cornetto_amd.bgzf_scan(got[1])[2]


@pytest.mark.parametrize("name", ["short_block", "cut_record", "fields_l_seq", "first_error_wins"])
def test_cli_malformed_file_leaves_a_cut_stream(cli, tmp_path, name):
    data, _ = fq.bad_cases()[name]
    p = tmp_path / (name + ".bam")
    p.write_bytes(bc.write(data, [150, 90, 120]))
    args = ["seq", "-m", "0", "--bam", str(p)]
    want = run(cli, args)
    assert want[0] == 1 and want[1] == fq.oracle(data).text and len(want[1]) > 0
    for env in ({}, {"CORNETTO_BAM_WINDOW": "400", "CORNETTO_EMIT_SLAB": "16"}):
        got = run(cli, args + ["--bgzf"], env)
        assert got[0] == 1 and lines_of(got[2]) == lines_of(want[2]) and len(lines_of(got[2])) == 1, (name, got[2][-1500:])
        assert not got[1].endswith(bc.EOF_BLOCK) and all(r[5] > 0 for r in bc.members(got[1]))
        assert b"".join(bc.inflate_members(got[1])) == want[1]
