"""CPU: bgzip- and gzip-compressed depth files of `(no)boringbits` on the host path (--accel=no: both kinds through zlib, cli/bgcomp.c), with the
product binary and with the host C under the sanitizers.  Everything is parity with the same command on the plain files: stdout, stderr
without the footer and the timing lines, exit status.  On the parent commit the compressed bytes are read as text and every command here
that is given a compressed file ends with "The depth files should have 4 columns" (--runs: "has 4 columns")."""
import gzip
import os
import threading

import pytest

import bgcomp_cases as bz
import bgzf_cases as bc
from helpers import PANEL, panel_argv
from runs_cases import to_runs
from test_cli_host import cli, run          # noqa: F401  (the product binary and the sanitized build of the same host C)

HOST = "--accel=no"
COMMANDS = [PANEL[4], PANEL[5], PANEL[14]]          # noboringbits and boringbits on cov-*, boringbits on sparse-*


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgcomp_host")
    texts = {fn: bz.golden_text(golden_dir, fn) for fn in bz.DEPTH_FILES}
    out = bz.write_variants(d, texts, seed=3)
    runs = bz.write_variants(d, {fn: to_runs(t, "max") for fn, t in texts.items()}, seed=5, lo=1, hi=900, tag="runs.")
    return out, runs


def mixed(v, kind, which):
    """the files of `kind` for cov-total ("t"), cov-mq ("q") or both ("tq"), the plain ones for the rest"""
    return {fn: (v[kind][fn] if ("total" in fn and "t" in which) or ("mq20" in fn and "q" in which) else v["plain"][fn]) for fn in v["plain"]}


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and bz.stderr_lines(a[2]) == bz.stderr_lines(b[2]), (a[0], b[0], bz.stderr_lines(a[2])[:4], bz.stderr_lines(b[2])[:4])


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
@pytest.mark.parametrize("which", ["tq", "t", "q"])
def test_host_compressed_equals_plain(cli, files, kind, which):        # noqa: F811
    per_base, runs = files
    for args, _ in COMMANDS:
        want = run(cli, panel_argv(per_base["plain"], args) + [HOST])
        assert want[0] == 0 and want[1]
        same(run(cli, panel_argv(mixed(per_base, kind, which), args) + [HOST]), want)
    args = COMMANDS[0][0]
    want = run(cli, panel_argv(runs["plain"], args) + [HOST, "--runs"])
    assert want[0] == 0 and want[1]
    same(run(cli, panel_argv(mixed(runs, kind, which), args) + [HOST, "--runs"]), want)


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_host_compressed_panel_equals_plain(cli, files, tmp_path, kind):        # noqa: F811
    per_base, _ = files
    lens = {}
    for ln in open(per_base["plain"]["cov-total.bg"], "rb"):
        f = ln.split()
        lens[f[0]] = int(f[2])
    (tmp_path / "asm.bed").write_bytes(b"".join(b"%s\t0\t%d\n" % (n, ln) for n, ln in lens.items()))
    opts = ["-w", "1000", "-i", "100", "-e", "2000", "-m", "10000", "--panel", str(tmp_path / "asm.bed"), "--panel-params", "300,2000,500,700,3000,2500,4000", HOST]
    want = run(cli, ["noboringbits", per_base["plain"]["cov-total.bg"], "-q", per_base["plain"]["cov-mq20.bg"]] + opts)
    assert want[0] == 0 and want[1]
    same(run(cli, ["noboringbits", per_base[kind]["cov-total.bg"], "-q", per_base[kind]["cov-mq20.bg"]] + opts), want)


def small_pair():
    vals = [(b"ctgA", [30 + (i * 7) % 11 for i in range(3000)]), (b"ctgB", [70000 if i == 5 else 12 for i in range(1500)])]
    return bz.per_base(vals), bz.per_base([(n, [v // 2 for v in x]) for n, x in vals])


SMALL_ARGS = ["-w", "100", "-i", "10", "-m", "500", "-e", "100", HOST]


def test_host_damaged_truncated_and_mixed_chains(cli, tmp_path):        # noqa: F811
    t, q = small_pair()
    (tmp_path / "q.bg").write_bytes(q)
    blob = bz.bgzf(t, bz.seeded_sizes(len(t), 1, 500, 3000), eof=False)
    k = 3
    off, _ = bz.block_offset(blob, k)
    bad = dict(bz.damaged(blob, k))
    bad["cut"] = blob[:off + 40]                                         # the file ends inside block 3
    bad["gzip_behind"] = blob + gzip.compress(b"ctgB\t1500\t1501\t3\n")  # a gzip member that is no BGZF member behind the chain
    for name, data in bad.items():
        p = tmp_path / ("bad_%s.bg.gz" % name.replace("+", "p").replace("-", "m"))
        p.write_bytes(data)
        for extra in ([], ["--runs"]):
            rc, out, err = run(cli, ["noboringbits", str(p), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS + extra)
            lines = [ln for ln in bz.stderr_lines(err) if "ERROR" in ln]
            assert rc == 1 and out == b"" and len(lines) == 1 and os.path.basename(str(p)) in lines[0], (name, extra, rc, lines)
            if name not in ("gzip_behind",):
                assert "block %d at offset %d" % (k, off) in lines[0], (name, lines)
    # a damaged gzip file (no BGZF): the same line without a block
    g = bytearray(gzip.compress(t))
    g[len(g) // 2] ^= 0x55
    (tmp_path / "bad.gz").write_bytes(bytes(g))
    rc, out, err = run(cli, ["noboringbits", str(tmp_path / "bad.gz"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS)
    lines = [ln for ln in bz.stderr_lines(err) if "ERROR" in ln]
    assert rc == 1 and out == b"" and len(lines) == 1 and "bad.gz" in lines[0]
    # a file without the EOF block is accepted
    (tmp_path / "t.bg").write_bytes(t)
    (tmp_path / "noeof.bg.gz").write_bytes(blob)
    want = run(cli, ["noboringbits", str(tmp_path / "t.bg"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS)
    assert want[0] == 0 and want[1]
    same(run(cli, ["noboringbits", str(tmp_path / "noeof.bg.gz"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS), want)


def test_host_text_errors_read_as_for_the_plain_file(cli, tmp_path):        # noqa: F811
    t, q = small_pair()
    tl, ql = t.splitlines(True), q.splitlines(True)
    cases = {
        "columns": (b"".join(tl[:700] + [b"ctgA\t700\t701\n"] + tl[701:]), q),
        "order": (t, b"".join(ql[:900] + ql[901:])),
        "increment": (b"".join(tl[:1200] + tl[1201:]), b"".join(ql[:1200] + ql[1201:])),
        "end": (b"".join(tl[:40] + [b"ctgA\t40\t45\t3\n"] + tl[41:]), b"".join(ql[:40] + [b"ctgA\t40\t45\t3\n"] + ql[41:])),
    }
    for name, (tt, qq) in cases.items():
        v = bz.write_variants(tmp_path, {"total.bg": tt, "mq20.bg": qq}, seed=9, lo=1, hi=700, tag=name + ".")
        want = run(cli, ["noboringbits", v["plain"]["total.bg"], "-q", v["plain"]["mq20.bg"]] + SMALL_ARGS)
        assert want[0] == 1 and want[1] == b"" and any("ERROR" in ln for ln in bz.stderr_lines(want[2])), name
        for kind in ("bgzf", "gzip"):
            same(run(cli, ["noboringbits", v[kind]["total.bg"], "-q", v[kind]["mq20.bg"]] + SMALL_ARGS), want)


def through_fifo(cli, tmp_path, data, q_path, name):        # noqa: F811
    import subprocess
    fifo = str(tmp_path / name)
    os.mkfifo(fifo)

    def feed():
        try:
            with open(fifo, "wb") as f:
                f.write(data)
        except BrokenPipeError:
            pass
    th = threading.Thread(target=feed)
    th.start()
    p = subprocess.run([cli, "noboringbits", fifo, "-q", q_path] + SMALL_ARGS, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    th.join()
    return p.returncode, p.stdout, p.stderr


def test_host_fifos_are_read_as_ever(cli, tmp_path):        # noqa: F811
    """a FIFO is never peeked into: plain text works, BGZF bytes are read as the text they are not"""
    t, q = small_pair()
    (tmp_path / "t.bg").write_bytes(t)
    (tmp_path / "q.bg").write_bytes(q)
    want = run(cli, ["noboringbits", str(tmp_path / "t.bg"), "-q", str(tmp_path / "q.bg")] + SMALL_ARGS)
    got = through_fifo(cli, tmp_path, t, str(tmp_path / "q.bg"), "plain.fifo")
    assert want[0] == 0 and got[0] == 0 and got[1] == want[1] and want[1]
    rc, out, err = through_fifo(cli, tmp_path, bc.write(t, sizes=[700, 900]), str(tmp_path / "q.bg"), "bgzf.fifo")
    assert rc == 1 and out == b"" and b"The depth files should have 4 columns" in err


def test_block_placement_and_packed_names_under_the_sanitizers(tmp_path):
    """tools/sim/bgsrc_sim.cc: the offsets a compressed source's blocks are inflated to and the indices of the bg_names kernel, in heap blocks of
    exactly the sizes the library asks for"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bgsrc_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tools", "sim", "bgsrc_sim.cc"), "-o", exe])
    p = subprocess.run([exe, "120"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith(b"bgsrc_sim: 120 seeds") and p.stdout.rstrip().endswith(b"ok"), p.stderr.decode()[-2000:]
