"""CPU: the hand-assembled deflate streams of tests/deflate_asm.py — zlib's inflate takes every valid one to the bytes expand() computed and
refuses every invalid one, the walker finds in every named case the shape it is there for, and all of them go as BGZF files through the
device's decoder on the CPU under AddressSanitizer + UBSan (tools/sim/inflate_sim.cc --status, the program tests/test_bgzf_host.py builds),
which gives every invalid stream the CNI_BAD_* reason aimed at.  tests/test_gpu_inflate_crafted.py runs the same streams on the device."""
import os
import subprocess
import zlib

import pytest

import bgzf_cases as bc
import deflate_asm as da
from test_bgzf_host import sim          # noqa: F401  (the fixture that builds the sanitized program)

VALID = da.valid_cases()
INVALID = da.invalid_cases()


def _zlib(payload):
    """-> (the stream ended, bytes out); raises zlib.error"""
    d = zlib.decompressobj(-15)
    got = d.decompress(payload)
    return d.eof, got


@pytest.mark.parametrize("name", da.singles() + ["tiny_blocks"])
def test_zlib_inflates_every_named_case_to_the_expected_bytes(name):
    payload, exp, check = VALID[name]
    eof, got = _zlib(payload)
    assert eof and got == exp and da.FILL not in exp
    w = bc.walk(payload)
    assert w["out"] == len(exp) and check(w), (name, w)


def _copy_grid_size():
    """p x len x the distinct distances of the recipe that lie in 1 .. p, and exact_end"""
    return 1 + sum(len({d for d in (1, 2, 3, 63, 64, 65, n - 1, n, n + 1, p) if 1 <= d <= p}) for p in (1, 63, 64, 65, 130) for n in da.LEN_EDGES)


@pytest.mark.parametrize("grid,n_members", [("fence_grid", 5 * 4), ("copy_grid", _copy_grid_size()), ("seeded", 300)])
def test_zlib_inflates_every_member_of_the_grids(grid, n_members):
    names = da.group(grid)
    assert len(names) == n_members
    for name in names:
        payload, exp, check = VALID[name]
        eof, got = _zlib(payload)
        assert eof and got == exp and da.FILL not in exp and len(exp) <= 65536, name
        w = bc.walk(payload)
        assert w["out"] == len(exp) and check(w), (name, w)
    assert len(VALID["copy_grid/exact_end"][1]) == 65536
    assert all(len(VALID[n][1]) <= 4096 for n in da.group("seeded"))


def test_the_seeded_members_cover_what_they_draw_from():
    """between them: every block kind, runs of each repeat code across HLIT, the three incomplete code sets inflate allows, 284 + 31,
    overlapping and far matches, 15-bit codes"""
    ws = [bc.walk(VALID[n][0]) for n in da.group("seeded")]
    assert {"stored", "fixed", "dynamic"} == {k for w in ws for k in w["kinds"]}
    assert {16, 17, 18} == {s for w in ws for s in w["run_over_hlit"]}
    assert {0, 1} <= {n for w in ws for n in w["n_dist_codes"]} and 1 in {n for w in ws for n in w["n_lit_codes"]}
    assert any(284 in w["len_syms"] and w["max_len"] == 258 for w in ws) and any(w["overlaps"] for w in ws)
    assert max(w["max_code_len"] for w in ws) == 15 and max(w["max_dist"] for w in ws) > 2048
    assert any(w["empty_stored"] for w in ws)


def test_expand_is_the_plain_copy():
    assert da.expand([1, 2, 3, (5, 2), 4, (3, 6)]) == bytes([1, 2, 3, 2, 3, 2, 3, 2, 4, 2, 3, 2])
    assert da.expand([(4, 1)], before=b"ab") == b"bbbb"
    for n in (1, 2, 3, 19, 286):
        assert da.kraft(da.flat(n)) == 32768 or n == 1
    assert da.len_sym(258) == 285 and da.len_sym(257) == 284 and da.len_sym(3) == 257 and da.dist_sym(32768) == 29 and da.dist_sym(1) == 0


@pytest.mark.parametrize("name", sorted(INVALID))
def test_zlib_refuses_every_invalid_case(name):
    payload, n_dst, reason = INVALID[name]
    try:
        eof, got = _zlib(payload)
    except zlib.error:
        return
    assert not (eof and len(got) == n_dst), name


def _files(d):
    """every case as a BGZF file: a named case a file, a grid a chain; the invalid ones with n_dst in the footer -> [(path, [names])]"""
    files = []
    for name in da.singles() + ["tiny_blocks"]:
        files.append((d / (name + ".gz"), [name]))
    for g in da.GROUPS:
        files.append((d / (g + ".gz"), da.group(g)))
    for path, names in files:
        path.write_bytes(b"".join(da.member_raw(VALID[n][0], VALID[n][1]) for n in names))
    bad = []
    for name in sorted(INVALID):
        payload, n_dst, _ = INVALID[name]
        bad.append((d / ("bad_" + name + ".gz"), [name]))
        bad[-1][0].write_bytes(da.member_raw(payload, isize=n_dst, crc=0))
    return files, bad


def test_every_case_through_the_decoder_under_the_sanitizers(sim):
    """inflate_sim --status --mut 50 over all crafted files: exit 0, no sanitizer report, no disagreement with zlib on any member, mutation,
    truncation or wrong size; status 0 for every valid member, and for every invalid one the reason aimed at — between them all of
    CNI_BAD_BLOCK .. CNI_BAD_INPUT"""
    exe, d = sim
    good, bad = _files(d)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, "--status", "--mut", "50", "--seed", "11"] + [str(f) for f, _ in good + bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "FAIL" not in err, (p.returncode, err[-3000:])
    status = {}
    for line in p.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "status":
            status[(w[1], int(w[2]))] = int(w[3])
    for path, names in good:
        for i, name in enumerate(names):
            assert status.pop((str(path), i)) == 0, name
    seen = set()
    for path, (name,) in bad:
        assert status.pop((str(path), 0)) == INVALID[name][2], name
        seen.add(INVALID[name][2])
    assert not status and seen == {da.BAD_BLOCK, da.BAD_CODES, da.BAD_SYMBOL, da.BAD_DISTANCE, da.BAD_LENGTH, da.BAD_INPUT}
