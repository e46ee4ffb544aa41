"""GPU: no stage depends on what its workspaces held before.  cn_selftest_ws_fill (development build, tests/selftest_bind.py) sets every byte
of every allocated workspace of a handle — device slots over their whole capacity, pinned slots too — and drops the vouchers of the two
slots whose contents a later call may rely on; the tile states of WS_SCAN / WS_STITCH, which kernels wait on, are the only thing it leaves
alone (tests/test_gpu_scan.py owns them).  DESIGN.md section 3 has the contract.

The protocol, the same for every stage S, every result compared bit for bit with the stage's reference (tests/ws_fill_cases.py: the oracle,
numpy, zlib, the plain-Python restatements), never with an earlier run:
  1. S(X) on a fresh handle: the first form of the stage;
  2. for each fill byte 0x00, 0xFF, 0xA5: fill, S(X) — the estimate-sized / one-go form where the stage has one (asserted through
     last_timing where the names tell);
  3. fill 0xFF, S(Y), S(X): a small call inside a large call's workspaces, then the large call behind it.
0x00 is what a fresh allocation usually holds, the one value under which an unwritten word reads as "count 0 / status OK / flag clear": it
must pass and alone would prove nothing.  0xFF makes every unwritten counter huge and every unwritten flag set; 0xA5 is neither extreme.
Every test has a handle of its own: a workspace never shrinks, and a handle that has seen a large input makes every fill large."""
import ctypes as C

import numpy as np
import pytest

import cornetto_amd
import selftest_bind as st
import sort_bind
import ws_fill_cases as wc

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
NEVER_FILLED = {"WS_SCAN", "WS_STITCH"}


@pytest.fixture
def acc():
    a = cornetto_amd.Accel(0, dev=True)
    yield a
    a.close()


def fill(acc, byte, uses=()):
    """fill, and what the report must say: nothing skipped but the polled slots, device and pinned bytes filled, the stage's own slots among them"""
    filled, skipped, pinned = st.ws_fill(acc, byte)
    assert set(skipped) <= NEVER_FILLED, skipped
    assert sum(filled.values()) > 0 and sum(pinned.values()) > 0, (filled, pinned)
    assert set(uses) <= set(filled) | set(pinned), sorted(set(uses) - set(filled) - set(pinned))
    return filled


def same(got, exp, what):
    ok = got == exp                    # (no diff of megabytes in the report)
    assert ok, what


def protocol(acc, name, run, uses=(), form=None):
    """steps 1-3 for the stage whose cases are wc.STAGES[name]; run(which) -> the stage's result for case "X" / "Y", exp(which) its reference;
    form(turn): the check of the stage's form after the turn-th S(X)"""
    assert wc.references_differ(name)
    X, Y = wc.STAGES[name]("X"), wc.STAGES[name]("Y")
    exp = lambda c: {k: v for k, v in c.items() if k.startswith("exp")}
    same(run("X"), exp(X), "the first call on a fresh handle")
    if form:
        form(1)
    for turn, byte in enumerate(FILLS, 2):
        fill(acc, byte, uses)
        same(run("X"), exp(X), "X after a fill with 0x%02X" % byte)
        if form:
            form(turn)
    fill(acc, 0xFF, uses)
    same(run("Y"), exp(Y), "Y inside X's workspaces filled with 0xFF")
    same(run("X"), exp(X), "X behind Y, no fill in between")


def names_of(acc):
    """the launch names of the most recent compute call, all of them (Accel.last_timing() stops at 64)"""
    n = acc.L.cornetto_accel_last_timing(acc.h, None, None, 0)
    nm, ms = (C.c_char_p * max(n, 1))(), (C.c_float * max(n, 1))()
    acc.L.cornetto_accel_last_timing(acc.h, nm, ms, n)
    return [x.decode() for x in nm[:n]]


# ---- the hook itself ----------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_slot_and_a_fresh_handle_has_nothing_to_fill(acc):
    classes = st.ws_classes()
    assert len(classes) == len(st.ws_names()) and {n for n, (c, _) in classes.items() if c == "polled"} == NEVER_FILLED
    assert all(v for _, (c, v) in classes.items() if c != "scratch") and all(v == "" for _, (c, v) in classes.items() if c == "scratch")
    assert st.ws_fill(acc, 0xFF) == ({}, {}, {})
    rc, _, _, _ = st.ws_fill_rc(acc, 256)
    assert rc == st.E_ARG


def test_fill_is_refused_while_a_lazy_handles_copies_are_out(acc):
    """a lazy handle returns when its kernels are through and copies the large results on a stream of its own: until wait() the call is not
    complete, and the hook touches nothing"""
    case = wc.cov("Y")
    w, inc = wc.COV_SETS[0]
    lo, hi = case["exp"]["thr"]
    acc.set_lazy(True)
    cov = acc.cov_upload(case["depths"], case["mqs"])
    assert acc.cov_prepare(cov, w, inc) == case["exp"]["sums"]
    recs = acc.cov_select(cov, lo, hi, wc.COV_SEL["Q"], wc.COV_SEL["edge"], wc.COV_SEL["min_len"], False)
    rc, filled, skipped, pinned = st.ws_fill_rc(acc, 0xFF)
    assert rc == st.E_ARG and not filled and not pinned
    acc.wait()
    assert recs.tobytes() == case["exp"][(w, inc, False)]
    fill(acc, 0xFF, ("WS_CW_SEL", "PIN_SMALL"))
    recs = acc.cov_select(cov, lo, hi, wc.COV_SEL["Q"], wc.COV_SEL["edge"], wc.COV_SEL["min_len"], False)
    acc.wait()
    assert recs.tobytes() == case["exp"][(w, inc, False)]
    cov.close()


# ---- telofind / telowin / telo_scan -----------------------------------------------------------------------------------------------------------
def telo_run(acc, asm, case):
    out = {}
    for m in wc.MOTIFS:                                        # (the motif changes from call to call: the tables of WS_TF_LUT with it)
        hits = acc.telofind(asm, m)
        wins = acc.telowin(hits, case["lens"], case["thr"])    # marks from a hit list: the WS_TW_* slots
        h2, w2 = acc.telo_scan(asm, m, case["thr"])             # the fused marks: WS_TF_BITMAP
        _, w3 = acc.telo_scan(asm, m, case["thr"], want_hits=False)
        e = (hits.tobytes(), wins.tobytes())
        assert (h2.tobytes(), w2.tobytes()) == e and w3.tobytes() == e[1], m
        out[m] = e
    return {"exp": out}


def test_telo(acc):
    """Y is another assembly (the voucher of the mark bitmap's padding) and X starts with the first motif again (the voucher of the tables)"""
    asm = {w: acc.asm_upload(wc.telo(w)["seqs"]) for w in "XY"}
    protocol(acc, "telo", lambda w: telo_run(acc, asm[w], wc.telo(w)),
             uses=("WS_TF_LUT", "WS_TF_BITMAP", "WS_TF_CNT", "WS_TF_TC", "WS_TF_TB", "WS_TF_RUNS", "WS_TF_HITS", "WS_TW_BITMAP", "WS_TW_OUT", "PIN_SMALL", "PIN_TW"))
    for a in asm.values():
        a.close()


def test_telo_scan_without_hits_of_a_motif_beyond_the_automaton(acc):
    """a motif of more than 32 bytes without a border is scanned by the sequential rule and writes no marks: the windows come from its runs
    whether or not the caller wants the runs"""
    case = wc.telo("Y")
    asm = acc.asm_upload(case["seqs"])
    _, wins = acc.telo_scan(asm, wc.LONG_MOTIF, case["thr"], want_hits=False)
    asm.close()
    assert wins.tobytes() == case["exp"][wc.LONG_MOTIF][1]


# ---- sdust ------------------------------------------------------------------------------------------------------------------------------------
SD_USES = ("WS_SD_OUT", "WS_SD_CNT", "WS_SD_OFF", "WS_SD_DST", "WS_SD_STATS", "PIN_SMALL")


SD_SETS = ((20, 64), (25, 40))


def sdust_asms(acc):
    """a resident assembly per case and parameter set: the counts a call leaves for the next one are kept with the assembly, for ONE (T, W)"""
    return {(w, tw): acc.asm_upload(wc.sdust(w)["seqs"]) for w in "XY" for tw in SD_SETS}


def sdust_run(acc, asm, w):
    return {"exp": {(T, W): acc.sdust(asm[(w, (T, W))], T, W).tobytes() for T, W in SD_SETS}}


def test_sdust_sift_and_its_one_go_form(acc):
    """the default family on the product's configuration.  The estimates live with the assembly, so every S(X) but the first is the one-go
    form: ONE launch named sdust_stitch (the fused merge) where the first form has one per kernel of the stepwise merge"""
    asm = sdust_asms(acc)
    stitches = []

    def run(w):
        got = sdust_run(acc, asm, w)
        stitches.append((w, names_of(acc).count("sdust_stitch")))      # (of the last call, T = 25, W = 40)
        return got

    def form(turn):
        w, n = stitches[-1]
        assert "sdust_kernel" in names_of(acc) and w == "X" and (n > 1 if turn == 1 else n == 1), stitches
    protocol(acc, "sdust", run, uses=SD_USES, form=form)
    assert stitches[-2][0] == "Y" and stitches[-2][1] > 1 and stitches[-1] == ("X", 1), stitches
    for a in asm.values():
        a.close()


@pytest.mark.parametrize("switch", ["CORNETTO_SDUST_SIFT=0", "CORNETTO_SDUST_VARIANT=1"])
def test_sdust_other_kernel_families(acc, monkeypatch, switch):
    """sdust_w64 (the per-lane recurrence with its plan, claim flags and slot rows) and sdust_kernel<RC> through the development switches"""
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    asm = sdust_asms(acc)
    protocol(acc, "sdust", lambda w: sdust_run(acc, asm, w), uses=SD_USES)
    for a in asm.values():
        a.close()


def test_sdust_begin_end_and_the_refused_fill(acc):
    """the fill in front of _begin only: between _begin and _end the call is queued on the stream and the hook refuses — E_ARG, nothing
    touched, and the pending call still ends with the right result"""
    case = wc.sdust("X")
    asm = acc.asm_upload(case["seqs"])
    exp = case["exp"][(20, 64)]
    assert acc.sdust(asm, 20, 64).tobytes() == exp
    for byte in FILLS:
        fill(acc, byte, SD_USES)
        before = acc.launch_count()
        acc.sdust_begin(asm, 20, 64)
        assert acc.launch_count() != before                              # queued: sized by the last call's counts
        rc, filled, skipped, pinned = st.ws_fill_rc(acc, 0xFF)
        assert rc == st.E_ARG and not filled and not pinned
        assert acc.sdust_end(asm, 20, 64).tobytes() == exp, byte
    asm.close()


def test_sdust_core_on_the_library_handle(acc):
    """cornetto_sdust_core() works on a handle the library keeps for itself (a new assembly per call: always the first form)"""
    L = acc.L
    buf = L.cornetto_sdust_buf_init(None)

    def run(w):
        s = wc.sdust_core(w)["seq"]
        n = C.c_int(-1)
        p = L.cornetto_sdust_core(s.ctypes.data_as(C.c_void_p), s.size, 20, 64, C.byref(n), buf)
        assert n.value >= 0
        return np.ctypeslib.as_array(p, shape=(n.value,)).tobytes()
    try:
        X, Y = wc.sdust_core("X"), wc.sdust_core("Y")
        assert wc.references_differ("sdust_core")
        assert run("X") == X["exp"]
        own = st.sdust_core_handle()
        for byte in FILLS:
            fill(own, byte, SD_USES)
            assert run("X") == X["exp"], byte
        fill(own, 0xFF, SD_USES)
        assert run("Y") == Y["exp"]
        assert run("X") == X["exp"]
    finally:
        L.cornetto_sdust_buf_destroy(buf)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------
def cov_run(acc, cov, case):
    out = {}
    Q, edge, min_len = wc.COV_SEL["Q"], wc.COV_SEL["edge"], wc.COV_SEL["min_len"]
    for w, inc in wc.COV_SETS:
        out["sums"] = acc.cov_prepare(cov, w, inc)
        mean = int(np.floor(out["sums"][0] / out["sums"][2] + 0.5))
        lo, hi = out["thr"] = (acc.cov_threshold(0.4, mean), acc.cov_threshold(2.5, mean))
        out[(w, inc, "regs")] = [acc.cov_regs(cov, c).tobytes() for c in case["probe"]]
        for boring in (False, True):
            recs = acc.cov_select(cov, lo, hi, Q, edge, min_len, boring)
            pk, cf = acc.cov_select_packed(cov, lo, hi, Q, edge, min_len, boring)
            assert acc.unpack_regs(pk, cf, case["lens"], w).tobytes() == recs.tobytes(), (w, inc, boring)
            out[(w, inc, boring)] = recs.tobytes()
            m = acc.cov_select_merged(cov, lo, hi, Q, edge, min_len, boring, 1000, 3000)
            out[(w, inc, boring, "merged")] = m.tobytes()
    return {"exp": out}


def test_coverage(acc):
    cov = {w: acc.cov_upload(wc.cov(w)["depths"], wc.cov(w)["mqs"]) for w in "XY"}
    protocol(acc, "cov", lambda w: cov_run(acc, cov[w], wc.cov(w)),
             uses=("WS_CB_T32", "WS_CB_T64", "WS_CB_GRAND", "WS_CW_REGS", "WS_CW_SEL", "WS_CW_CNT", "WS_CW_TRES", "WS_CW_CF", "WS_CW_MERGE", "PIN_SMALL", "PIN_CW"))
    for c in cov.values():
        c.close()


# ---- bedgraph ingest and the run-length expansion ------------------------------------------------------------------------------------------------
def bedgraph_run(acc, case):
    """complete sessions (the fills stand between them, never between two feeds): both readers, the text in three pieces"""
    res = []
    for reader, (t, q) in ((acc.bedgraph_ingest, case["per_base"]), (acc.bedgraph_runs_ingest, case["runs"])):
        cut = lambda x: [p for p in (x[:len(x) // 3], x[len(x) // 3:len(x) // 3 + 5000], x[len(x) // 3 + 5000:]) if p]
        cov, names, ncl = reader(cut(t), cut(q))
        try:
            got = (names, ncl, [tuple(a.tobytes() for a in acc.cov_download(cov, c)) for c in range(len(names))])
        finally:
            cov.close()
        res.append(got)
    assert res[0] == res[1]
    return {"exp": res[0]}


def test_bedgraph_ingest_and_runs(acc):
    protocol(acc, "bedgraph", lambda w: bedgraph_run(acc, wc.bedgraph(w)), uses=("WS_BG_TEXT_A", "WS_BG_TEXT_B", "WS_BG_SMALL", "PIN_SMALL"))


# ---- telomere breaks and ends -----------------------------------------------------------------------------------------------------------------
def triples(rows):
    return [(int(r["ctg"]), int(r["start"]), int(r["finish"])) for r in rows]


def test_telobreaks_on_lists(acc):
    def run(w):
        c = wc.breaks_lists(w)
        lens = np.array(c["lens"], np.int32)
        sd, tel = np.array(c["sd"], dtype=cornetto_amd.IVL_DT), np.array(c["tel"], dtype=cornetto_amd.TELROW_DT)
        a, b = triples(acc.telobreaks_ivl(lens, sd, tel)), triples(acc.telobreaks(lens, sd, tel))
        assert a == b
        return {"exp": a}
    protocol(acc, "breaks_lists", run, uses=("WS_TB", "WS_TB_SMALL", "WS_TB_OUT", "PIN_SMALL"))


def test_telo_breaks_and_telo_ends(acc):
    asm = {w: acc.asm_upload([r[1] for r in wc.breaks_asm(w)["records"]]) for w in "XY"}
    thr = acc.telowin_threshold(0.4, 99.9)

    def run(w):
        return {"exp_breaks": triples(acc.telo_breaks(asm[w], b"TTAGGG", 20, 64)), "exp_ends": triples(acc.telo_ends(asm[w], b"TTAGGG", thr, 100, 5000))}
    protocol(acc, "breaks_asm", run, uses=("WS_TB_OUT", "WS_TB_SMALL", "WS_TE_WORDS", "WS_TE_CNT", "WS_SD_OUT", "WS_TF_BITMAP", "PIN_SMALL", "PIN_TE"))
    for a in asm.values():
        a.close()


# ---- FASTA / FASTQ framing -----------------------------------------------------------------------------------------------------------------------
def fastx_run(acc, case):
    fq, fa = case["fq"], case["fa"]
    recs, used, plain, _ = acc.fastq_split(fq, final=True)
    assert used == len(fq) and plain
    got_fq = []
    for r in recs:
        h, nl, cl, n = int(r["head"]), int(r["name_len"]), int(r["comment_len"]), int(r["len"])
        got_fq.append((fq[h + 1:h + 1 + nl], fq[h + nl + 2:h + nl + 2 + cl] if cl else b"", fq[int(r["seq"]):int(r["seq"]) + n], fq[int(r["qual"]):int(r["qual"]) + n]))
    recs, used, plain, seqs = acc.fasta_split(fa, final=True, want_seqs=True)
    assert used == len(fa) and plain
    got_fa = [(fa[int(r["head"]) + 1:int(r["head"]) + 1 + int(r["name_len"])], int(r["len"])) for r in recs]
    iv = acc.sdust(seqs, 20, 64).tobytes()          # the bases the framing moved into the resident layout
    seqs.close()
    return {"exp_fq": got_fq, "exp_fa": got_fa, "exp_seqs": iv}


def test_fasta_and_fastq_split(acc):
    protocol(acc, "fastx", lambda w: fastx_run(acc, wc.fastx(w)), uses=("WS_FQ_TEXT", "WS_FQ_RECS", "WS_FQ_ENDS", "WS_FQ_SRC", "PIN_SMALL"))


# ---- the interval stage -----------------------------------------------------------------------------------------------------------------------
def merge_run(acc, c):
    got = acc.ivl_merge(c["iv"], c["dist"])
    out = np.zeros(len(got), wc.ob.SPAN_DT)
    out["ctg"], out["start"], out["end"] = got["ctg"], got["start"], got["finish"]
    return {"exp": out.tobytes()}


def hap_run(acc, c):
    return {"exp": triples(acc.hap_fun(c["lens"], c["rows"], merge_dist=c["D"], flank=c["F"]))}


def sort_run(acc, c):
    k, v = sort_bind.sort_pairs(acc, c["keys"], np.arange(c["keys"].size, dtype=np.uint32), c["bits"])
    return {"exp": (k.tobytes(), v.tobytes())}


def test_hap_fun_ivl_merge_sort_pairs(acc):
    """one stage: the sort on its own (cn_selftest_sort_pairs) touches no pinned slot"""
    def run(w):
        got = {"exp_hap": hap_run(acc, wc.hap(w))["exp"]}
        assert {"hp_sort_pos", "hp_sort_query", "hp_block_merge", "hp_corners", "hp_gap_write", "hp_fun_merge"} <= set(names_of(acc))
        got["exp_merge"] = merge_run(acc, wc.merge(w))["exp"]
        got["exp_sort"] = sort_run(acc, wc.sort(w))["exp"]
        return got
    protocol(acc, "interval", run, uses=("WS_SORT", "WS_HAP_ROWS", "WS_HAP_BLOCKS", "WS_HAP_FUN", "WS_IVL_MERGE", "PIN_SMALL"))


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------------------------
def bgzf_fasta(acc, c):
    recs, used, plain, _, names = acc.fasta_split_bgzf(c["fa_blob"], final=True, want_names=True)
    assert plain and len(names) == len(recs)
    return [(n, int(r["len"])) for n, r in zip(names, recs)]


def bgzf_run(acc, c):
    """inflate with a bad block (its index, the status, every other block's bytes and every canary byte), the framed text with its names through
    text_gather (empty ranges among them), then inflate again: WS_BZ_BLOCKS serves both"""
    got, first_bad = acc.bgzf_inflate(c["bad"], blocks=c["blocks"], fill=0xA5)
    assert (first_bad, acc.last_status) == (c["bad_at"], -6)
    assert {"bgzf_inflate", "bgzf_crc32"} <= {n for n, _ in acc.inflate_timing}
    free = np.ones(len(got), dtype=bool)
    for i, b in enumerate(c["blocks"]):
        d, n = int(b["dst"]), int(b["n_dst"])
        free[d:d + n] = False
        if i != c["bad_at"]:
            assert got[d:d + n] == c["parts"][i], i
    assert free.sum() >= 64 * len(c["blocks"]) + 256 and bytes(np.frombuffer(got, dtype=np.uint8)[free]) == b"\xa5" * int(free.sum())
    fa = bgzf_fasta(acc, c)
    text, first_bad = acc.bgzf_inflate(c["good"])
    assert first_bad == -1 and acc.last_status == 0 and text == c["good_text"]
    return {"exp_fa": fa}


def test_bgzf_inflate_gather_inflate(acc):
    protocol(acc, "bgzf", lambda w: bgzf_run(acc, wc.bgzf(w)), uses=("WS_BZ_BLOCKS", "WS_BZ_STATUS", "WS_BZ_PACK", "WS_FQ_RECS", "PIN_SMALL"))


# ---- the panel step -----------------------------------------------------------------------------------------------------------------------------
def test_panel_step(acc):
    """S = two steps in a row, both against the reference.  The telomere side tells its form by the order of its launches: the exact call
    needs the list totals on the host before the windows (tf_order in front of tw_scan), the queued one launches the windows right behind
    the scan.  Behind a fill the tables of the motif are gone with their voucher, so the queued scan declines and the exact call uploads
    them — its documented behaviour; the step after that is queued again."""
    obj = {w: (acc.asm_upload(wc.step(w)["seqs"]), acc.cov_upload(wc.step(w)["depths"], wc.step(w)["mqs"])) for w in "XY"}
    P = wc.STEP
    forms = []

    def one(w):
        c = wc.step(w)
        sums, thr, pk, cf, hits, wins = acc.panel_step(obj[w][0], obj[w][1], P["motif"], c["thr"], P["w"], P["inc"], P["low_cov"], P["high_cov"], P["low_mq"], P["edge_len"],
                                                       P["min_ctg_len"], False)
        nm = names_of(acc)
        forms.append("queued" if nm.index("tw_scan") < nm.index("tf_order") else "exact")
        return sums, thr, acc.unpack_regs(pk, cf, c["lens"], P["w"]).tobytes(), hits.tobytes(), wins.tobytes()

    def run(w):
        a, b = one(w), one(w)
        assert a == b
        return {"exp": a}

    def form(turn):
        assert forms[-2:] == ["exact", "queued"], forms
    protocol(acc, "step", run, uses=("WS_TF_LUT", "WS_TF_BITMAP", "WS_CW_SEL", "WS_CW_CF", "WS_TW_OUT", "PIN_STEP", "PIN_TW", "PIN_CW"), form=form)
    for a, c in obj.values():
        a.close()
        c.close()


# ---- one chain across the stages that share WS_SCAN (never filled), WS_SORT and PIN_SMALL -----------------------------------------------------------
def test_chain_across_stages(acc):
    steps = [("hap", lambda: hap_run(acc, wc.hap("X"))["exp"], wc.hap("X")["exp"]),
             ("merge", lambda: merge_run(acc, wc.merge("X"))["exp"], wc.merge("X")["exp"]),
             ("breaks_lists", lambda: triples(acc.telobreaks_ivl(np.array(wc.breaks_lists("X")["lens"], np.int32), np.array(wc.breaks_lists("X")["sd"], dtype=cornetto_amd.IVL_DT),
                                                                 np.array(wc.breaks_lists("X")["tel"], dtype=cornetto_amd.TELROW_DT))), wc.breaks_lists("X")["exp"]),
             ("sort", lambda: sort_run(acc, wc.sort("X"))["exp"], wc.sort("X")["exp"]),
             ("bgzf", lambda: bgzf_fasta(acc, wc.bgzf("X")), wc.bgzf("X")["exp_fa"])]
    for rnd, bytes_ in enumerate(((0xFF, 0xA5, 0x00, 0xFF, 0xA5), (0xA5, 0xFF, 0xFF, 0x00, 0xFF))):
        for (name, run, exp), byte in zip(steps, bytes_):
            same(run(), exp, "%s in round %d" % (name, rnd))
            fill(acc, byte)
