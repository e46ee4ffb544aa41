"""Shared by tests/test_telobreaks_rule.py and tests/test_gpu_telobreaks_ivl.py: what `cornetto telostats --breaks`, cornetto_telo_breaks()
and cornetto_telobreaks_ivl() must give.

    the interval rule (rule): src/telomere_breaks.c:95-148 of the reference for a low-complexity list that is sorted with every start beyond
        the previous finish — a row of at least 24 bases marks the one interval, cut at the contig length L, that contains
        [max(0, start - 100), min(L, end + 100)); a marked interval prints once as max(start - 1, 0) to min(finish, L) - 1;
    the chain (chain_rows, breaks_text): test/realtest.sh:65-69 on top of the oracle (tests/oracle_bind.py, pinned to the reference) —
        sdust and telofind per record, the bitsets of telobreaks, the contigs in the bucket order of the reference's khash table;
    a generator of short records with planted low-complexity blocks, and a CLI runner."""
import bisect
import os

import numpy as np

import oracle_bind as ob
import telostats_cases as tc

HOST = tc.HOST
MIN_TEL, FLANK = 24, 100


# ---- the rule on intervals ---------------------------------------------------------------------------------------------------------------
def rule(ctg_len, sd, tel):
    """ctg_len: lengths; sd: [(ctg, start, finish)] by (ctg, start), start > previous finish inside a contig; tel: [(ctg, start, end, matched)]
    -> [(ctg, first - 1 clamped at 0, last)] by (ctg, start)"""
    keys = [(c << 32) | s for c, s, _ in sd]
    marked = set()
    for c, s, e, m in tel:
        if m < MIN_TEL or not 0 <= c < len(ctg_len):
            continue
        L = ctg_len[c]
        a, b = max(0, s - FLANK), min(L, e + FLANK)
        i = bisect.bisect_right(keys, (c << 32) | a) - 1          # the last interval that starts at or before a
        if i < 0 or sd[i][0] != c:
            continue
        if min(sd[i][2], L) >= b:
            marked.add(i)
    return [(sd[i][0], max(sd[i][1] - 1, 0), min(sd[i][2], ctg_len[sd[i][0]]) - 1) for i in sorted(marked)]


def precondition(sd):
    """every start beyond the previous finish inside a contig, contigs in order"""
    return all(p[0] < v[0] or (p[0] == v[0] and v[1] > p[2]) for p, v in zip(sd, sd[1:]))


# ---- the chain on the oracle -------------------------------------------------------------------------------------------------------------
def oracle_sdust(seq, T=20, W=64):
    """[(start, finish)] of one record"""
    return [(int(v >> 32), int(v & 0xFFFFFFFF)) for v in ob.sdust(seq, T, W)] if len(seq) else []


def oracle_lists(records, m=b"TTAGGG", T=20, W=64):
    """-> (lens, sd [(ctg, start, finish)], tel [(ctg, start, end, matched)]) as the three text files of the chain hold them"""
    lens, sd, tel = [], [], []
    for ci, (_, seq) in enumerate(records):
        lens.append(len(seq))
        sd += [(ci, s, f) for s, f in oracle_sdust(seq, T, W)]
        tel += [(ci, int(h["start"]), int(h["end"]), int(h["end"] - h["start"])) for h in ob.telofind(seq, m)] if len(seq) else []
    return lens, sd, tel


def oracle_bitset(lens, sd, tel):
    """the reference's two bitsets (orc_telobreaks) -> [(ctg, first, last)]"""
    out = ob.telobreaks(np.array(lens, np.int32), np.array(sd, dtype=ob.SPAN_DT) if sd else np.zeros(0, ob.SPAN_DT),
                        np.array(tel, dtype=ob.TELROW_DT) if tel else np.zeros(0, ob.TELROW_DT))
    assert out is not None, "coordinates outside a contig"
    return [(int(r["ctg"]), int(r["start"]), int(r["end"])) for r in out]


def chain_rows(records, m=b"TTAGGG", T=20, W=64):
    return oracle_bitset(*oracle_lists(records, m, T, W))


def chain_rows_threaded(records, m=b"TTAGGG", T=20, W=64, threads=8):
    """chain_rows() for a large assembly: the per-record lists on a few threads (the oracle calls release the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda r: oracle_lists([r], m, T, W), records))
    lens = [p[0][0] for p in parts]
    sd = [(ci, s, f) for ci, p in enumerate(parts) for _, s, f in p[1]]
    tel = [(ci, s, e, k) for ci, p in enumerate(parts) for _, s, e, k in p[2]]
    return oracle_bitset(lens, sd, tel)


def breaks_text(records, rows):
    """the lines of `telobreaks` (src/telomere_breaks.c:133-148): contigs in khash bucket order (names must differ), rows by position"""
    names = [r[0] for r in records]
    assert len(set(names)) == len(names)
    _, order = ob.khash_order(names)
    per = {}
    for c, s, e in rows:
        per.setdefault(c, []).append((s, e))
    return b"".join(b"Found telomere positions %d to %d is a telomere in %s of length %d\n" % (s, e, names[c], len(records[c][1]))
                    for c in (int(x) for x in order) for s, e in per.get(c, []))


# ---- sequences -----------------------------------------------------------------------------------------------------------------------------
def random_record(rng, max_len=6000):
    """0 to max_len random bases with planted TTAGGG / CCCTAA / AC / poly-A / N blocks, more of them at the two ends, then substitutions
    inside the blocks, single N and lower case"""
    L = int(rng.integers(0, max_len + 1))
    s = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes())
    for _ in range(int(rng.integers(0, 7))) if L else []:
        n = int(rng.choice([30, 80, 150, 260, 400, 900, 2000]))
        a = int(rng.choice([0, max(0, L - n)])) if rng.random() < 0.35 else int(rng.integers(0, L))
        b = min(L, a + n)
        unit = [b"TTAGGG", b"TTAGGG", b"CCCTAA", b"AC", b"A", b"N"][int(rng.integers(0, 6))]
        blk = bytearray((unit * ((b - a) // len(unit) + 1))[:b - a])
        if rng.random() < 0.6 and b > a:                                  # substitutions: a base, or a single N
            for p in rng.integers(0, b - a, size=(b - a) // int(rng.integers(20, 200)) + 1):
                blk[int(p)] = b"ACGTN"[int(rng.integers(0, 5))]
        s[a:b] = blk
    if L and rng.random() < 0.3:                                          # a lower-case stretch: both scans fold the case
        a = int(rng.integers(0, L))
        b = min(L, a + int(rng.integers(1, 500)))
        s[a:b] = bytes(s[a:b]).lower()
    return bytes(s)


def sample(n, seed=7):
    """n generated records with the sdust parameters each one is scanned with: [(seq, T, W)]"""
    rng = np.random.default_rng(seed)
    # (the oracle's sdust takes 0.2 s per record at W = 128 and a hundredth of that at 32: the wide window for one record in sixteen)
    return [(random_record(rng), int(rng.choice([10, 20, 30])), int(rng.choice([20, 32, 64, 128], p=[5 / 16, 5 / 16, 5 / 16, 1 / 16]))) for _ in range(n)]


def thinned_telomere(n, every=150, unit=b"TTAGGG"):
    """a telomere block with one substitution every `every` bases: runs of about `every` bases whose flanks are low-complexity too"""
    blk = bytearray(tc.telomere(n, unit))
    for p in range(every // 2, n, every):
        blk[p] = ord("C") if blk[p] != ord("C") else ord("A")
    return bytes(blk)


def planted_thin(rng, L, blocks, unit=b"TTAGGG", every=150):
    """a record of L bases: background with thinned telomere blocks over every [a, b) of `blocks` (a perfect block between random flanks is
    ONE run whose flanks are not low-complexity: no break)"""
    s = bytearray(tc.background(rng, L))
    for a, b in blocks:
        s[a:b] = thinned_telomere(b - a, every, unit)
    return bytes(s)


def random_assembly(rng, max_len=130_000):
    """1-6 records of 0 to max_len bases (tests/telostats_cases.py) with some of the generator's low-complexity blocks on top"""
    recs = []
    for name, seq in tc.random_assembly(rng, max_len):
        s = bytearray(seq)
        for _ in range(int(rng.integers(0, 4))) if len(s) > 3000 else []:
            a = int(rng.integers(0, len(s) - 2500))
            blk = random_record(rng, 2500)
            s[a:a + len(blk)] = blk
        recs.append((name, bytes(s)))
    return recs


def random_soup(rng):
    """explicit lists: 1-6 contigs of 0 to 5000 bases, disjoint sorted intervals (gaps of one base among them, the last one of a contig now and
    then beyond the contig's end) and rows — inside intervals, their flanks on and around the interval's edges, and anywhere — -> (lens, sd, tel)"""
    lens, sd, tel = [], [], []
    for c in range(int(rng.integers(1, 7))):
        L = int(rng.choice([0, 1, 150, 5000])) if rng.random() < 0.2 else int(rng.integers(0, 5001))
        lens.append(L)
        mine, pos = [], int(rng.integers(0, 60))
        while pos < L:
            f = pos + int(rng.choice([5, 60, 230, 260, 400, 900]))
            if f > L:
                f = L if rng.random() < 0.5 else L + int(rng.integers(1, 65))
            mine.append((c, pos, f))
            pos = f + int(rng.choice([1, 1, 2, 30, 300]))
        sd += mine
        for _ in range(int(rng.integers(0, 12))) if L > 30 else []:
            n = int(rng.choice([23, 24, 25, 40, 120]))
            if mine and rng.random() < 0.7:
                _, s, f = mine[int(rng.integers(0, len(mine)))]
                st = (s + FLANK + int(rng.choice([-1, 0, 0, 1, 7]))) if rng.random() < 0.5 else (min(f, L) - FLANK - n + int(rng.choice([-7, -1, 0, 0, 1])))
            else:
                st = int(rng.integers(0, L))
            st = max(0, min(st, L - n))
            if 0 <= st < st + n <= L:
                tel.append((c, st, st + n, n))
    return lens, sd, tel


# ---- the records of the CLI tests --------------------------------------------------------------------------------------------------------------
def cli_records():
    rng = np.random.default_rng(61)
    return [(b"both", planted_thin(rng, 30000, [(0, 3000), (27500, 30000)], every=400)), (b"none", tc.background(rng, 8000)), (b"empty", b""),
            (b"right", planted_thin(rng, 16001, [(14000, 16001)], b"CCCTAA", 90)), (b"whole", tc.telomere(4200)),
            (b"thin", planted_thin(rng, 20000, [(6000, 11000)]))]


def write_inputs(d, records):
    (d / "asm.fa").write_bytes(tc.fasta(records))
    (d / "asm.fq").write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in records))
    (d / "asm.lens").write_bytes(b"".join(b"%s\t%d\n" % (n, len(s)) for n, s in records))


def expected_text(records):
    """the oracle chain's file, with the properties the records are there for"""
    lens, sd, tel = oracle_lists(records)
    rows = oracle_bitset(lens, sd, tel)
    assert rows == rule(lens, sd, tel)
    per = [sum(r[0] == c for r in rows) for c in range(len(records))]
    assert per[0] >= 2 and per[1] == 0 and per[2] == 0 and per[3] >= 1, per            # a record without runs between two with runs, an empty one
    assert [r for r in rows if r[0] == 4] == [(4, 0, 4199)]                              # the fully telomeric record: one break over all of it
    # the thinned block: rows in its interior mark with BOTH flanks inside the low-complexity interval (neither clipped at 0 or L)
    L = lens[5]
    inner = [(s, e) for c, s, e, m in tel if c == 5 and m >= 24 and s - 100 > 0 and e + 100 < L and
             any(v[0] == 5 and v[1] <= s - 100 and min(v[2], L) >= e + 100 for v in sd)]
    assert len(inner) >= 10 and per[5] >= 1, (inner, per)
    text = breaks_text(records, rows)
    assert text.count(b"\n") == len(rows) > 0
    return text


def shared_name_case():
    """the CLI records and a seventh record that carries the name of the first -> (records, the file --breaks writes for them): the lines of
    the two records in record order at the place of the name in the khash order, each with its own length"""
    records = cli_records()
    records.append((records[0][0], records[0][1][:5000]))
    names = [r[0] for r in records]
    slot, order = ob.khash_order(names)
    per = [chain_rows([r]) for r in records]
    assert per[0] and per[6] and len(records[6][1]) != len(records[0][1])
    text = b"".join(b"Found telomere positions %d to %d is a telomere in %s of length %d\n" % (s, e, names[i], len(records[i][1]))
                    for k in order for i in range(len(records)) if slot[i] == k for _, s, e in per[i])
    return records, text


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
def run_breaks(cli, path, cwd, env=None, opts=()):
    """`cornetto telostats <opts> -b out.bed --breaks out.breaks path` in cwd under env -> dict(rc, out, err, bed, breaks)"""
    for f in ("out.bed", "out.breaks"):
        if os.path.exists(os.path.join(cwd, f)):
            os.remove(os.path.join(cwd, f))
    got = tc.run_cli(cli, ["telostats"] + list(opts) + ["-b", "out.bed", "--breaks", "out.breaks", path], cwd, env)
    for f, k in (("out.bed", "bed"), ("out.breaks", "breaks")):
        p = os.path.join(cwd, f)
        got[k] = open(p, "rb").read() if os.path.exists(p) else None
    return got
