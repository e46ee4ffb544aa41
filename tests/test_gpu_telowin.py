"""GPU: telowin on explicit hit lists and on the marks of the telofind pass, every window compared with the oracle (tests/telowin_cases.py).

The other tests of this stage hand cornetto_telowin() telofind output (disjoint per strand, sorted, a multiple of the motif long) and compare,
under one positive threshold, only the windows that pass.  Here the hits overlap, repeat, come unsorted, are one base long, lie inside one
64-bit word or end / start on its boundary (tw_fill: `lo == 0`, `hi == 64`, several workgroups); the contig lengths sit on the seams of the
visiting rule (1000, 1200, ...), of the block clip at the contig's end and of the 256-window tile (52 000 / 52 001); and thr_adj = 0 returns
`car` of EVERY window the reference's loop visits (src/telomere_windows.c:31-41), so a wrong count shows whether or not it changes a verdict.
Ties pin `>=` at car / den == thr.  The same seams run through the fused scan and the panel step (marks written by tf_scan), and thousands
of one-window contigs take the result copy of run_tw_scan_dev beyond its speculative rows and through its exact retry.  Exact integer and
byte comparisons throughout."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cornetto_amd
import oracle_bind as ob
import telowin_cases as twc
from helpers import golden

pytestmark = pytest.mark.gpu

E_ARG = -3                 # CORNETTO_E_ARG (include/cornetto_accel.h)
# run_tw_scan_dev (csrc/telo.hip): `spec`, the rows copied together with the count, and the `cap` of WS_TW_OUT on a handle that has not
# allocated it yet (1u << 16) — more windows than that and the kernel runs a second time with the exact size
SPEC_ROWS = 16384
FIRST_CAP = 1 << 16

# (threshold, identity) as the command line takes them; identity None: thr_adj as given.  0: every visited window; 1.5: none
THRESHOLDS = [(0.0, None), (0.4, 99.9), (0.1, 90.0), (0.8, 99.9), (1.5, None)]


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def thr_adj(acc, thr, identity):
    if identity is None:
        return thr
    t = acc.telowin_threshold(thr, identity)
    assert t == ob.telowin_threshold(thr, identity)
    return t


def same(got, exp, what=""):
    """equal rows; the first difference by name (no diff of thousands of rows in the report)"""
    assert got.dtype == exp.dtype, (got.dtype, exp.dtype)
    if len(got) == len(exp) and np.array_equal(got, exp):
        return
    k = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    assert False, "%s: %d rows against %d expected; first difference at row %d: got %s, expected %s" % (
        what, len(got), len(exp), k, got[k] if k < len(got) else None, exp[k] if k < len(exp) else None)


def names_of(acc):
    """the launch names of the most recent compute call, all of them (Accel.last_timing() stops at 64)"""
    n = acc.L.cornetto_accel_last_timing(acc.h, None, None, 0)
    nm, ms = (C.c_char_p * max(n, 1))(), (C.c_float * max(n, 1))()
    acc.L.cornetto_accel_last_timing(acc.h, nm, ms, n)
    return [x.decode() for x in nm[:n]]


@functools.lru_cache(maxsize=None)
def seam_expected(whole, t):
    return twc.expected(twc.seam_contigs(whole), t)


# ---- cornetto_telowin: tw_fill + tw_scan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,identity", THRESHOLDS)
@pytest.mark.parametrize("whole", [False, True])
def test_seam_contigs(acc, whole, thr, identity):
    """every seam length under overlapping, repeated, unsorted, one-base and empty hits; the same marks from the sorted list and from the
    list with every hit twice give the same rows (bits are OR-ed, never added)"""
    t = thr_adj(acc, thr, identity)
    case, exp = twc.seam_contigs(whole), seam_expected(whole, t)
    if t == 0:
        assert len(exp) == sum(twc.n_windows(int(n)) for n in case["lens"])
        assert not whole or np.array_equal(exp["car"], exp["end"] - exp["start"])
    elif t > 1:
        assert len(exp) == 0
    else:
        assert 0 < len(exp)
    same(acc.telowin(case["hits"], case["lens"], t), exp, "as given")
    assert "tw_fill" in names_of(acc) and "tw_scan" in names_of(acc)
    for how, v in twc.variants(case).items():
        same(acc.telowin(v["hits"], v["lens"], t), exp, how)


def test_ties(acc):
    """car / den == thr passes, one mark less (or one base more) does not: 500 / 1000, 499 / 1000, 300 / 600, 300 / 601 at 0.5"""
    case = twc.tie_contigs()
    t = thr_adj(acc, *twc.TIE)
    assert t == 0.5
    same(acc.telowin(case["hits"], case["lens"], t), twc.expected(case, t), "ties")
    same(acc.telowin(case["hits"], case["lens"], 0.0), twc.expected(case, 0.0), "every window of the tie contigs")


# ---- the marks of the telofind pass -------------------------------------------------------------------------------------------------------
def test_seams_through_the_fused_scan(acc):
    """runs of the motif that end on, start on and straddle 64 k, 200 k and 51 200: the marks come from tf_scan, the windows from the
    assembly's own tile layout; thr 0, a real threshold and thr 0 again on one handle and one assembly"""
    seqs = twc.seam_assembly()
    asm = acc.asm_upload(seqs)
    try:
        for t in (0.0, thr_adj(acc, 0.4, 99.9), 0.0):
            eh, ew = twc.expected_scan(seqs, t)
            assert len(eh) > 300 and len(ew) > 50
            hits, wins = acc.telo_scan(asm, twc.MOTIF, t)
            nm = names_of(acc)
            assert "tf_scan" in nm and "tw_scan" in nm and "tw_fill" not in nm, nm      # (the fused marks, not a list of hits)
            same(hits, eh, "hits at %r" % t)
            same(wins, ew, "windows at %r" % t)
    finally:
        asm.close()


def test_seams_through_the_panel_step(acc):
    """one step at thr 0 and the same step again: the second is queued in one go, its window copy sized by the first step's count, and
    returns the same windows — all of them (tests/test_gpu_step.py has the step against the four calls under a positive threshold)"""
    seqs = [s for s in twc.seam_assembly() if len(s)]             # (the coverage side wants a position in every contig)
    rng = np.random.default_rng(9)
    depths = [rng.integers(0, 60, size=len(s)).astype(np.uint16) for s in seqs]
    mqs = [(d // 2).astype(np.uint16) for d in depths]
    eh, ew = twc.expected_scan(seqs, 0.0)
    asm, cov = acc.asm_upload(seqs), acc.cov_upload(depths, mqs)
    try:
        forms = []
        for _ in range(2):
            sums, thr, pk, cf, hits, wins = acc.panel_step(asm, cov, twc.MOTIF, 0.0, 500, 50, 0.6, 1.4, 0.7, 1000, 5000, False)
            nm = names_of(acc)
            forms.append("queued" if nm.index("tw_scan") < nm.index("tf_order") else "exact")
            same(hits, eh, "hits of the %s step" % forms[-1])
            same(wins, ew, "windows of the %s step" % forms[-1])
        assert forms == ["exact", "queued"], forms
    finally:
        asm.close()
        cov.close()


# ---- the result copy of run_tw_scan_dev -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ctg,launches", [(20000, 1), (70000, 2)])
def test_more_windows_than_the_speculative_copy_holds(n_ctg, launches):
    """a handle of its own: the window workspace keeps its size within a handle, and only on a fresh one is the path the one named.
    20 000 windows: the rows beyond the 16 384 copied with the count are fetched, one launch; 70 000: more than the first workspace
    holds, tw_scan runs again with the exact size.  Then a small call on the same handle."""
    assert SPEC_ROWS < 20000 <= FIRST_CAP < 70000 and n_ctg in (20000, 70000)
    case = twc.many_windows(n_ctg)
    exp = twc.expected(case, 0.0)
    assert len(exp) == n_ctg and int(exp["car"].sum()) == len(case["hits"]) == (n_ctg + 2) // 3
    a = cornetto_amd.Accel(0)
    try:
        got = a.telowin(case["hits"], case["lens"], 0.0)
        assert names_of(a).count("tw_scan") == launches
        same(got, exp, "%d windows" % n_ctg)
        small = twc.tie_contigs()
        same(a.telowin(small["hits"], small["lens"], 0.5), twc.expected(small, 0.5), "a small call behind it")
        assert names_of(a).count("tw_scan") == 1
    finally:
        a.close()


# ---- what the ABI refuses -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,msg", [
    ((3, 0, 0, 10), "telowin: hit 4 names contig 3 of 3"),
    ((-1, 0, 0, 10), "telowin: hit 4 names contig -1 of 3"),
    ((0, 1, -1, 10), "telowin: hit 4 [-1,10) lies outside contig 0 of length 3000"),
    ((1, 0, 590, 601), "telowin: hit 4 [590,601) lies outside contig 1 of length 600"),
])
def test_refusals(acc, bad, msg):
    """a hit outside the table of contigs or outside its contig (the reference writes out of bounds there): CORNETTO_E_ARG with the message
    of telowin_from_hits, nothing marked, and the handle is good for the next call"""
    case = twc.tie_contigs()
    hits = np.insert(case["hits"], 4, np.array([bad], dtype=twc.HIT))
    with pytest.raises(cornetto_amd.AccelError) as ei:
        acc.telowin(hits, case["lens"], 0.0)
    assert ei.value.status == E_ARG and msg in str(ei.value), str(ei.value)
    same(acc.telowin(case["hits"], case["lens"], 0.0), twc.expected(case, 0.0), "the valid call behind the refusal")


# ---- the command line on the device path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("identity,thr,exp", [
    ("100", "0", "hits_craft.i100t0.telowin.exp"),
    ("100", "0.5", "hits_craft.i100t05.telowin.exp"),
    ("99.9", "0.4", "hits_craft.telowin.exp"),
    ("90", "0.1", "hits_craft.i90t01.telowin.exp"),
])
def test_cli_on_the_crafted_hit_list(golden_dir, identity, thr, exp):
    """`cornetto telowin` (parser -> cornetto_telowin -> printf) prints what the unmodified reference prints on the fixture of
    tests/golden/make_golden_telowin_hits.py, and says the reference's line on stderr"""
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    env = {k: v for k, v in os.environ.items() if k != "CORNETTO_ACCEL"}
    p = subprocess.run([cornetto_amd.CLI_PATH, "telowin", os.path.join(golden_dir, "hits_craft.telomere"), identity, thr],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout == golden(golden_dir, exp)
    assert twc.stderr_line(identity, thr) in p.stderr
