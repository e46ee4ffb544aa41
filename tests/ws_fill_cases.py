"""The inputs of tests/test_gpu_ws_fill.py and their references, made on the host only (the oracle, numpy, zlib, the plain-Python restatements
of the stages' own tests).  Per stage two inputs: X, the smallest on which every kernel of the stage runs and every device scan in it
sees more than one tile, and Y, smaller and of another shape.  Every function is cached: a reference is computed once per process."""
import functools

import numpy as np

import bgzf_cases as zc
import cornetto_amd
import hap_cases as hc
import oracle_bind as ob
import runs_cases as rc
import telobreaks_cases as bc
import telostats_cases as tc
from helpers import token_at, tricky_fastx

SCAN_TILE = 4096           # cnscan::SC_TILE: counters per tile of the device scans
TF_TILE = 16256            # telo.hip: positions per telofind tile
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
IVL, HIT, WIN = cornetto_amd.IVL_DT, cornetto_amd.HIT_DT, cornetto_amd.WIN_DT

cached = functools.lru_cache(maxsize=None)


def revcomp(m):
    return m[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def has_border(m):
    return any(m[:k] == m[-k:] for k in range(1, len(m)))


# ---- telofind / telowin / telo_scan ------------------------------------------------------------------------------------------------------------
LONG_MOTIF = b"ACGTTGCAAGCTTAGGCATCGATCCGTAAGCTTGG"           # longer than the 32 bytes of the automaton, and without a border
MOTIFS = (b"TTAGGG", b"AAAA", LONG_MOTIF)
assert len(LONG_MOTIF) > 32 and not has_border(LONG_MOTIF) and not has_border(revcomp(LONG_MOTIF)) and has_border(b"AAAA") and not has_border(b"TTAGGG")


def _telo_seqs(which):
    rng = np.random.default_rng(31 if which == "X" else 32)
    seqs = []
    # X: as test_telofind_more_tiles_than_one_scan_tile_vs_oracle builds them — every contig is a telofind tile of its own, 4100 of them are
    # two tiles of tf_order's scan; Y: a few dozen
    for i in range(4100 if which == "X" else 37):
        n = int(rng.integers(6, 41))
        s = ACGT[rng.integers(0, 4, size=n)].copy()
        if i % 3 != 1:
            m = MOTIFS[i % 2]
            unit = (m, revcomp(m))[(i // 2) % 2]
            p = int(rng.integers(0, n - len(m) + 1))
            rep = np.frombuffer(unit * int(rng.integers(1, 5)), dtype=np.uint8)[: n - p]
            s[p:p + len(rep)] = rep
        seqs.append(s)
    # and contigs with windows of their own: telomere blocks at the ends, arrays of the long motif and of poly-A inside
    for k, n in enumerate((21_000, 5300, 1001) if which == "X" else (7000, 999)):
        s = ACGT[rng.integers(0, 4, size=n)].copy()
        blocks = [(0, min(n, 1800), b"CCCTAA"), (max(0, n - 1300), n, b"TTAGGG"), (n // 2, min(n, n // 2 + 400), LONG_MOTIF), (n // 3, min(n, n // 3 + 90), b"A"),
                  (n // 4, min(n, n // 4 + 150), revcomp(LONG_MOTIF))]
        for a, b, unit in blocks[k % 2:]:
            s[a:b] = np.frombuffer((unit * ((b - a) // len(unit) + 1))[:b - a], dtype=np.uint8)
        seqs.insert(int(rng.integers(0, len(seqs))), s)
    return seqs


@cached
def telo(which):
    seqs = _telo_seqs(which)
    thr = ob.telowin_threshold(0.4, 99.9)
    exp = {}
    for m in MOTIFS:
        hits, wins = [], []
        for ci, s in enumerate(seqs):
            oh = ob.telofind(s, m)
            hits += [(ci, int(h["strand"]), int(h["start"]), int(h["end"])) for h in oh]
            wins += [(ci, int(w["start"]), int(w["end"]), int(w["car"])) for w in ob.telowin(oh, len(s), thr)]
        assert hits and wins, m
        exp[m] = (np.array(hits, dtype=HIT).tobytes(), np.array(wins, dtype=WIN).tobytes())
    n_tiles = sum((len(s) + TF_TILE - 1) // TF_TILE for s in seqs)
    assert (n_tiles > SCAN_TILE) == (which == "X")
    return {"seqs": seqs, "lens": np.array([len(s) for s in seqs], np.int32), "thr": thr, "exp": exp}


# ---- sdust ---------------------------------------------------------------------------------------------------------------------------------
def _plant(rng, s, n_blocks):
    for _ in range(n_blocks):
        unit = [b"A", b"AT", b"CAG", b"TTAGGG", b"N", b"acgt", b"AACCCT"][int(rng.integers(0, 7))]
        rep = np.frombuffer(unit * int(rng.integers(8, 120)), dtype=np.uint8)
        p = int(rng.integers(0, max(1, len(s) - 10)))
        s[p:p + len(rep)] = rep[:len(s[p:p + len(rep)])]


def _sdust_seqs(which):
    rng = np.random.default_rng(41 if which == "X" else 42)
    seqs = []
    if which == "X":
        # 4150 contigs are 4150 chunks and more: two tiles of the scan of the chunks' counts (sdust_scan), of the walk list's ranks (sdust_order)
        for i in range(4150):
            s = ACGT[rng.integers(0, 4, size=int(rng.integers(30, 260)))].copy()
            if i % 4 == 0:
                _plant(rng, s, 1)
            seqs.append(s)
        big = [90_000, 40_000, 20_011]
    else:
        big = [23_000, 9000, 70, 3]
    for n in big:
        s = ACGT[rng.integers(0, 4, size=n)].copy()
        _plant(rng, s, max(1, n // 700))
        if n > 10_000:                         # a repeat array over several chunks (the dp tiles of the sift) and a run of N (the walk list)
            s[n // 2:n // 2 + 6000] = np.frombuffer((b"CATTC" * 1200)[:6000], dtype=np.uint8)
            s[n // 5:n // 5 + 2500] = ord("N")
        seqs.insert(int(rng.integers(0, len(seqs) + 1)), s)
    return seqs


def sdust_rows(seqs, T, W):
    rows = [(ci, int(v) >> 32, int(v) & 0xFFFFFFFF) for ci, s in enumerate(seqs) if len(s) for v in ob.sdust(s, T, W)]
    return np.array(rows, dtype=IVL).reshape(-1)


@cached
def sdust(which):
    seqs = _sdust_seqs(which)
    exp = {(T, W): sdust_rows(seqs, T, W).tobytes() for T, W in ((20, 64), (25, 40))}
    assert all(exp.values()) and exp[(20, 64)] != exp[(25, 40)]
    return {"seqs": seqs, "exp": exp}


@cached
def sdust_core(which):
    """one sequence for the buffered interface: the reference's result words (start << 32 | finish)"""
    seqs = _sdust_seqs(which)
    s = np.concatenate([x for x in seqs if len(x) > 5000][:2])
    exp = np.array([int(v) for v in ob.sdust(s, 20, 64)], dtype=np.uint64)
    assert exp.size > 10
    return {"seq": s, "exp": exp.tobytes()}


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
COV_SETS = ((2500, 50), (300, 7))           # the default, and w % inc != 0: the heads of the blocks are written
COV_SEL = dict(Q=0.4, edge=100, min_len=20)


def _cov_arrays(which):
    rng = np.random.default_rng(51 if which == "X" else 52)
    # X: a contig has a window tile per 256 windows and at least one — 4200 short contigs and three long ones are more than one tile of
    # cov_order's scan, and with -w 300 -i 7 the long ones are thousands of block tiles
    lens = ([int(n) for n in rng.integers(30, 200, size=4200)] + [260_000, 61_003, 33_333]) if which == "X" else [52_000, 9000, 2501, 40]
    lens = [n for n in lens if all(ob.regs_assert(n, w, inc) == 0 for w, inc in COV_SETS)]
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    depths, mqs = [], []
    for n in lens:
        d = rng.poisson(30, size=(n + 499) // 500).repeat(500)[:n].astype(np.uint16)
        for _ in range(n // 20_000):
            a = int(rng.integers(0, n))
            d[a:a + int(rng.integers(500, 9000))] = rng.choice([2, 120])
        depths.append(d)
        mqs.append(np.minimum(d, rng.integers(0, 45, size=n)).astype(np.uint16))
    return lens, depths, mqs


@cached
def cov(which):
    lens, depths, mqs = _cov_arrays(which)
    sd, sq, n = sum(int(d.astype(np.int64).sum()) for d in depths), sum(int(q.astype(np.int64).sum()) for q in mqs), sum(lens)
    mean = int(np.floor(sd / n + 0.5))
    lo, hi = ob.threshold(0.4, mean), ob.threshold(2.5, mean)
    Q, edge, min_len = COV_SEL["Q"], COV_SEL["edge"], COV_SEL["min_len"]
    exp = {"sums": (sd, sq, n), "thr": (lo, hi)}
    probe = [int(np.argmax(lens)), len(lens) - 1, 0]           # the contigs whose windows are fetched one by one (cov_regs)
    for w, inc in COV_SETS:
        regs = [ob.get_regs(d, q, w, inc) for d, q in zip(depths, mqs)]
        exp[(w, inc, "regs")] = [regs[c].astype(cornetto_amd.REG_DT).tobytes() for c in probe]
        for boring in (False, True):
            rows = []
            for ci, r in enumerate(regs):
                L = lens[ci]
                if not ((L > min_len) if boring else (L >= min_len)):
                    continue
                for x in r:
                    st, end, dep, mq = int(x["st"]), int(x["end"]), int(x["depth"]), int(x["mq_depth"])
                    fun = bool(ob.is_fun(dep, mq, lo, hi, Q))
                    if (st > edge and end < L - edge and not fun) if boring else fun:
                        rows.append((ci, st, end, dep, mq))
            assert len(rows) > 20, (w, inc, boring)
            exp[(w, inc, boring)] = np.array(rows, dtype=cornetto_amd.REGREC_DT).tobytes()
            spans = np.array([r[:3] for r in rows], dtype=ob.SPAN_DT)
            m = ob.ivl_merge(spans, 1000)
            m = m[m["end"] - m["start"] >= 3000]
            exp[(w, inc, boring, "merged")] = m.tobytes()
        assert exp[(w, inc, False, "merged")] or exp[(w, inc, True, "merged")]
        n_tiles = sum((ob.n_reg(L, w, inc) + 255) // 256 for L in lens if L >= min_len)
        assert (n_tiles > SCAN_TILE) == (which == "X")
    return {"lens": lens, "depths": depths, "mqs": mqs, "probe": probe, "exp": exp}


# ---- bedgraph ingest (per base) and run-length expansion ----------------------------------------------------------------------------------------
@cached
def bedgraph(which):
    """a pair of run-length files (other run boundaries in the second) with a token at a tile seam of the tokeniser, X with more fresh records
    in one feed than a tile of the 64-bit offset scan holds (2048); the per-base reader gets their expansion, again with a token at the seam"""
    if which == "X":
        contigs = [[(1 + i % 3, (7 * i) % 60) for i in range(2100)], [(3 * cornetto_amd.BGRUN_TILE + 1, 33)], [(5, 65535), (400, 65536), (2, 70000), (40, 9)],
                   [(1 + i % 5, i % 50) for i in range(300)]]
    else:
        contigs = [[(1 + i % 7, (3 * i) % 40) for i in range(420)], [(700, 70000), (3, 1)]]

    def text_of(runs_of, cut=None):
        recs = []
        for ci, runs in enumerate(runs_of):
            n, p = sum(ln for ln, _ in runs), 0
            if cut:
                runs = [(min(cut, n - a), (3 * ci + a // cut) % 50) for a in range(0, n, cut)]
            for ln, v in runs:
                recs.append((b"contig_%d" % ci, p, p + ln, v))
                p += ln
        return rc.fmt(recs)
    def seam(text, at):                        # (Y's run-length files are shorter than a tile of the tokeniser)
        return token_at(text, at) if len(text) > 2 * at else text
    t, q = seam(text_of(contigs), 4095), seam(text_of(contigs, 37), 4096)
    names, ed, cl_t = rc.expand_arrays(t)
    qn, eq, cl_q = rc.expand_arrays(q)
    assert names == qn and [len(x) for x in ed] == [len(x) for x in eq] and len(rc.parse(t)) > (2048 if which == "X" else 100)
    exp = (names, cl_t + cl_q, [(d.tobytes(), m.tobytes()) for d, m in zip(ed, eq)])
    return {"runs": (t, q), "per_base": (token_at(rc.expand(t), 4095), token_at(rc.expand(q), 4096)), "exp": exp}


# ---- telomere breaks and ends ----------------------------------------------------------------------------------------------------------------
@cached
def breaks_lists(which):
    """explicit lists for cornetto_telobreaks / cornetto_telobreaks_ivl: X has more intervals than a tile of the scan of the marks"""
    if which == "X":
        lens, sd, tel = [], [], []
        for c, k in enumerate((1500, 1500, 1400)):
            lens.append(400 * k)
            sd += [(c, 400 * i, 400 * i + 300) for i in range(k)]
            tel += [(c, 400 * i + 120, 400 * i + 160, 40) for i in range(c, k, 3)]
        assert len(sd) > SCAN_TILE
    else:
        lens, sd, tel = bc.random_soup(np.random.default_rng(3))
    exp = bc.rule(lens, sd, tel)
    assert exp and bc.precondition(sd) and bc.oracle_bitset(lens, sd, tel) == exp
    return {"lens": lens, "sd": sd, "tel": tel, "exp": exp}


@cached
def breaks_asm(which):
    """records for cornetto_telo_breaks / cornetto_telo_ends (their scans take one tile per 4096 sdust intervals / mark words: an assembly of
    tens of megabases would be needed for two, so these stay at one — the lists above cover the scan of the marks)"""
    if which == "X":
        records = bc.cli_records()
    else:
        rng = np.random.default_rng(61)
        records = [(b"y0", bc.planted_thin(rng, 9000, [(0, 1500)], every=200)), (b"y1", tc.telomere(2100, b"CCCTAA")), (b"y2", tc.background(rng, 700))]
    rows = bc.chain_rows(records)
    ends = tc.expected(records, E=5000)["rows"]
    assert rows and ends
    return {"records": records, "exp_breaks": rows, "exp_ends": ends}


# ---- FASTA / FASTQ framing -----------------------------------------------------------------------------------------------------------------------
@cached
def fastx(which):
    rng = np.random.default_rng(71 if which == "X" else 72)
    n_rec = 260 if which == "X" else 9
    fq = tricky_fastx(rng, n_rec, strict=True)
    if not fq.endswith(b"\n"):
        fq += b"\n"
    assert not fq.endswith((b"+\n", b"+\r\n"))                                 # (an empty last read whose empty quality line went with the newline)
    recs, _ = ob.fastx_parse(tricky_fastx(rng, n_rec, strict=True, lowc=0.5))
    fa = b"".join(b">" + n + (b" " + c if c else b"") + b"\n" + b"".join(s[k:k + 61] + b"\n" for k in range(0, len(s), 61))
                  for n, c, s, _ in ((n, c.replace(b"\r", b""), s.replace(b"\r", b""), q) for n, c, s, q in recs))
    assert (len(fq) > 3 * 4096 and len(fa) > 3 * 4096) == (which == "X")       # records cross the 4096-byte tiles of the newline index
    efq, _ = ob.fastx_parse(fq)
    efa, _ = ob.fastx_parse(fa)
    assert len(efq) == n_rec and len(efa) == n_rec
    return {"fq": fq, "fa": fa, "exp_fq": [(n, c, s, q) for n, c, s, q in efq], "exp_fa": [(n, len(s)) for n, _, s, _ in efa],
            "exp_seqs": sdust_rows([np.frombuffer(s, dtype=np.uint8) for _, _, s, _ in efa], 20, 64).tobytes()}


# ---- the interval stage: merge, haplotype funbits, the sort ----------------------------------------------------------------------------------------
@cached
def merge(which):
    n = 5000 if which == "X" else 50           # X: five tiles of the max-scan (1024 intervals), two of the add-scan of the heads (4096)
    rng = np.random.default_rng(n)
    ctg = np.sort(rng.integers(0, n // 1000 + 3, size=n)).astype(np.int32)
    start = rng.integers(0, 5_000_000, size=n).astype(np.int32)
    order = np.lexsort((start, ctg))
    iv = np.zeros(n, IVL)
    iv["ctg"], iv["start"] = ctg[order], start[order]
    iv["finish"] = iv["start"] + rng.integers(0, 3000, size=n).astype(np.int32)
    iv["finish"][n // 2] = iv["start"][n // 2] + 400_000
    spans = np.zeros(n, ob.SPAN_DT)
    spans["ctg"], spans["start"], spans["end"] = iv["ctg"], iv["start"], iv["finish"]
    exp = ob.ivl_merge(spans, 10)
    assert 10 < len(exp) < n
    return {"iv": iv, "dist": 10, "exp": exp.tobytes()}


@cached
def hap(which):
    if which == "X":                           # the planted_small shape of test_gpu_hap.py: blocks, corners and gaps past the merge and the scan tile
        lens, haps, D, F = hc.planted_case(6000, 20, 1, queries_per_hap=60, D=50, max_len=3000, F=20)
        parts = [hc.hap_funbits(lens, rows, D, F) for rows in haps]
        assert sum(len(p[0]) for p in parts) > SCAN_TILE and sum(p[2] for p in parts) > SCAN_TILE
    else:
        lens, haps, D, F = hc.random_case(4)
    exp = hc.hap_fun(lens, haps, D, F)
    assert len(exp) > (100 if which == "X" else 1)
    return {"lens": lens, "rows": hc.to_device_rows(haps), "D": D, "F": F, "exp": exp}


@cached
def sort(which):
    import sort_bind
    n = (sort_bind.SCAN_TILE // 256) * sort_bind.SO_TILE + 1 + sort_bind.SO_TILE if which == "X" else 1500     # N_TABLE + T of test_gpu_hap.py
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    keys[::7] = keys[3]                        # equal keys: the order of their payloads is the input order
    order = np.argsort(keys, kind="stable")
    return {"keys": keys, "bits": 40, "exp": (keys[order].tobytes(), order.astype(np.uint32).tobytes())}


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------------------------
@cached
def bgzf(which):
    """X: the six-block file of test_gpu_bgzf.py with a payload byte of block 3 zeroed, laid out with canaries; a FASTA text of several blocks
    with empty names (two in a row among them); the six good blocks.  Y: two blocks, four records."""
    if which == "X":
        blob, cut = zc.bad_block_files()[3]
        good_text, good = zc.six_blocks()
        blocks, resume, broken = cornetto_amd.bgzf_scan(blob)
        assert len(blocks) == 6 and resume == len(blob) and not broken
        bad_at = 3
        rng = np.random.default_rng(81)
        recs = []
        for i in range(900):
            name = b"" if i % 5 in (1, 2) or i == 899 else b"n%d" % i          # ... two empty names in a row, and the last one
            recs.append(b">" + name + (b" c%d" % i if i % 3 == 0 and name else b"") + b"\n" + ACGT[rng.integers(0, 4, size=int(rng.integers(0, 150)))].tobytes() + b"\n")
        fa = b"".join(recs)
        fa_blob = zc.write(fa, sizes=[20_000, 1, 30_000, 9000])
    else:
        good_text = b">a\nACGT\n>\n>\nTTAGGGTTAGGG\n>b x\n\n>c\n" + zc.acgt(3000, 5) + b"\n"
        good = zc.write(good_text, sizes=[1500], eof=False)
        blob = bytearray(good)
        off, size, pay, n_pay, crc, isize = zc.members(good)[1]
        blob[off + size - 8] ^= 1                                              # the footer CRC of the second block of two
        blob, bad_at = bytes(blob), 1
        blocks, resume, broken = cornetto_amd.bgzf_scan(blob)
        fa, fa_blob = good_text, good
    blocks = blocks.copy()
    blocks["dst"] += 64 * np.arange(1, len(blocks) + 1)                        # 64 bytes of canary in front of every block
    efa, _ = ob.fastx_parse(fa)
    assert any(n == b"" and m == b"" for (n, _, _, _), (m, _, _, _) in zip(efa, efa[1:]))
    return {"bad": blob, "blocks": blocks, "bad_at": bad_at, "parts": zc.inflate_members(good), "good": good, "good_text": good_text,
            "fa_blob": fa_blob, "exp_fa": [(n, len(s)) for n, _, s, _ in efa]}


# ---- the panel step ------------------------------------------------------------------------------------------------------------------------------
STEP = dict(motif=b"TTAGGG", w=500, inc=50, low_cov=0.6, high_cov=1.4, low_mq=0.7, edge_len=1000, min_ctg_len=5000)


@cached
def step(which):
    """the bench's step in miniature (the workload of test_gpu_step.py): an assembly and its coverage, both strands' telomere units"""
    rng = np.random.default_rng(91 if which == "X" else 92)
    lens = ([int(x) for x in rng.integers(40_000, 90_000, size=4)] + [700, 64, 1]) if which == "X" else [31_000, 6000]
    seqs, depths, mqs = [], [], []
    for n in lens:
        s = ACGT[rng.integers(0, 4, size=n)].copy()
        for _ in range(max(1, n // 600)):
            p = int(rng.integers(0, max(1, n - 200)))
            rep = np.frombuffer((b"TTAGGG" if rng.random() < 0.5 else b"CCCTAA") * int(rng.integers(1, 40)), dtype=np.uint8)
            s[p:p + len(rep)] = rep[:len(s[p:p + len(rep)])]
        if n > 3000:
            s[:1800] = np.frombuffer(b"CCCTAA" * 300, dtype=np.uint8)
            s[-1200:] = np.frombuffer(b"TTAGGG" * 200, dtype=np.uint8)
        seqs.append(s)
        d = rng.poisson(30, size=(n + 499) // 500).repeat(500)[:n].astype(np.uint16)
        depths.append(d)
        mqs.append(np.minimum(d, rng.integers(0, 45, size=n)).astype(np.uint16))
    P = STEP
    thr = ob.telowin_threshold(0.4, 99.9)
    sd, sq, n = sum(int(d.astype(np.int64).sum()) for d in depths), sum(int(q.astype(np.int64).sum()) for q in mqs), sum(lens)
    mean = int(np.floor(sd / n + 0.5))
    lo, hi = ob.threshold(P["low_cov"], mean), ob.threshold(P["high_cov"], mean)
    rows, hits, wins = [], [], []
    for ci, (s, d, q) in enumerate(zip(seqs, depths, mqs)):
        if len(s) >= P["min_ctg_len"]:
            rows += [(ci, int(x["st"]), int(x["end"]), int(x["depth"]), int(x["mq_depth"])) for x in ob.get_regs(d, q, P["w"], P["inc"])
                     if ob.is_fun(int(x["depth"]), int(x["mq_depth"]), lo, hi, P["low_mq"])]
        oh = ob.telofind(s, P["motif"])
        hits += [(ci, int(h["strand"]), int(h["start"]), int(h["end"])) for h in oh]
        wins += [(ci, int(w["start"]), int(w["end"]), int(w["car"])) for w in ob.telowin(oh, len(s), thr)]
    assert len(rows) > 50 and len(hits) > 20 and len(wins) > 2
    exp = ((sd, sq, n), (lo, hi), np.array(rows, dtype=cornetto_amd.REGREC_DT).tobytes(), np.array(hits, dtype=HIT).tobytes(), np.array(wins, dtype=WIN).tobytes())
    return {"lens": lens, "seqs": seqs, "depths": depths, "mqs": mqs, "thr": thr, "exp": exp}


@cached
def interval(which):
    """the three of the interval stage as one: the sort on its own touches no pinned slot"""
    return {"exp_hap": hap(which)["exp"], "exp_merge": merge(which)["exp"], "exp_sort": sort(which)["exp"]}


STAGES = {"interval": interval, "telo": telo, "sdust": sdust, "sdust_core": sdust_core, "cov": cov, "bedgraph": bedgraph, "breaks_lists": breaks_lists, "breaks_asm": breaks_asm,
          "fastx": fastx, "merge": merge, "hap": hap, "sort": sort, "bgzf": bgzf, "step": step}


def references_differ(name):
    """X and Y of a stage give different, non-empty references"""
    x, y = STAGES[name]("X"), STAGES[name]("Y")
    keys = [k for k in x if k.startswith("exp")]
    assert keys
    for k in keys:
        assert x[k] and y[k] and repr(x[k]) != repr(y[k]), (name, k)
    return True
