"""Shared by tests/test_telostats_host.py and tests/test_gpu_telostats.py: what `cornetto telostats` (and cornetto_telo_ends) must give, restated
from scripts/telostats.sh:35-56 of the reference on top of the oracle's telofind / telowin (tests/oracle_bind.py, pinned to the reference):

    telofind | telowin I t | bedtools merge -d d | bedtools intersect -wa -b <end intervals> | cut -f1 | sort | uniq -c | awk

`bedtools merge` is a plain sequential sweep here (the product's device stage uses a run-length rule on one bit per window, its host path a
sweep of its own); `bedtools intersect -wa` prints a region once per end interval it shares at least one base with.  Also: a word-level model
of the device's run rule (run_rule) for the CPU test of that rule, sequence builders for the planted cases, the BED / stdout formatters and
a CLI runner."""
import os
import subprocess

import numpy as np

import oracle_bind as ob

HOST = {"CORNETTO_ACCEL": "no", "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}
MASK = (1 << 64) - 1


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def windows(seq, m=b"TTAGGG", t=0.4, I=99.9):
    """the qualifying windows [(start, end)] of one record: telofind, then telowin with the adjusted threshold"""
    thr = ob.telowin_threshold(t, I)
    wins = ob.telowin(ob.telofind(seq, m), len(seq), thr)
    return [(int(w["start"]), int(w["end"])) for w in wins]


def merge(wins, d):
    """bedtools merge -d d over intervals sorted by start: one sweep"""
    out = []
    for s, e in wins:
        if out and s <= out[-1][1] + d:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


def end_intervals(L, E):
    """scripts/telostats.sh:44"""
    return [(0, E), (L - E, L)] if L > 2 * E else [(0, L)]


def ends_rows(regions, L, E):
    """bedtools intersect -wa: A once per B it overlaps (B rows of one contig never overlap each other)"""
    return [(s, e) for s, e in regions for a, b in end_intervals(L, E) if s < b and e > a]


def expected(records, m=b"TTAGGG", t=0.4, I=99.9, d=100, E=50000):
    """records: [(name bytes, seq bytes)] -> dict(rows [(record index, start, end)], c per record, total, one, two, more, regions per record)"""
    rows, cs, regs = [], [], []
    for ci, (_, seq) in enumerate(records):
        r = merge(windows(seq, m, t, I), d)
        mine = ends_rows(r, len(seq), E)
        regs.append(r)
        cs.append(len(mine))
        rows += [(ci, s, e) for s, e in mine]
    return {"rows": rows, "c": cs, "regions": regs, "total": sum(cs), "one": sum(c == 1 for c in cs), "two": sum(c == 2 for c in cs),
            "more": sum(c > 2 for c in cs)}


def bed_text(records, exp):
    return b"".join(b"%s\t%d\t%d\n" % (records[ci][0], s, e) for ci, s, e in exp["rows"])


def prefix_of(path):
    """basename FILE .fa, then .fasta (scripts/telostats.sh:20-21)"""
    p = os.path.basename(path)
    for sfx in (".fa", ".fasta"):
        if p.endswith(sfx) and len(p) > len(sfx):
            p = p[:-len(sfx)]
    return p


def default_bed_name(path, t="0.4", E=50000):
    return "%s.windows.%s.%skb.ends.bed" % (prefix_of(path), t, "%.0f" % (E / 1000))


def stdout_text(path, exp, t="0.4", d=100, E=50000):
    """the script's stdout without its first (`cornetto --version`) line"""
    return ("genome: %s\nTHRESHOLD: %s\nends: %d\nasm: %s\nMerge telomere motifs in %dbp\n\nFind those at end of scaffolds, within < %d\n"
            "FILE\t%s\ntotal telomere regions at the end of contigs:\t%d\n\n\n"
            "contigs with 1 telo:\t%d\ncontigs with 2 telo:\t%d\ncontigs with more than 2 telo:\t%d\n\n"
            % (prefix_of(path), t, E, path, d, E, path, exp["total"], exp["one"], exp["two"], exp["more"])).encode()


# ---- the run rule of the device stage, word by word ----------------------------------------------------------------------------------------
def visited(L):
    """number of windows the loop of src/telomere_windows.c:31-41 visits: j = 0 .. the first j with 200 j + 1000 >= L"""
    return (L - 1000 + 199) // 200 + 1 if L > 1000 else 1


def window_of(j, L):
    return 200 * j, min(200 * j + 1000, L)


def _reach_back(hi, lo, k):
    hi, lo = ((hi << 1) | (lo >> 63)) & MASK, (lo << 1) & MASK
    w = 1
    while w < k:
        s = min(w, k - w)
        hi = (hi | (hi << s) | (lo >> (64 - s))) & MASK
        lo = (lo | (lo << s)) & MASK
        w += s
    return hi


def _brev(x):
    return int("{:064b}".format(x)[::-1], 2)


def run_rule(q, L, d):
    """q: one bool per visited window -> the merged regions by the run-length rule on 64-bit words (csrc/telostats.hip: te_runs, te_place):
    G = (1000 + d) / 200; head = q and no q in [j - G, j - 1]; tail = q and no q in [j + 1, j + G]; r-th head with r-th tail"""
    G = (1000 + d) // 200
    assert 1 <= G <= 63
    nw = (len(q) + 63) // 64
    words = [sum(1 << b for b in range(64) if 64 * w + b < len(q) and q[64 * w + b]) for w in range(nw)]
    heads, tails = [], []
    for w, cur in enumerate(words):
        prev = words[w - 1] if w > 0 else 0
        nxt = words[w + 1] if w + 1 < nw else 0
        hd = cur & ~_reach_back(cur, prev, G) & MASK
        tl = cur & ~_brev(_reach_back(_brev(cur), _brev(nxt), G)) & MASK
        heads += [64 * w + b for b in range(64) if hd >> b & 1]
        tails += [64 * w + b for b in range(64) if tl >> b & 1]
    assert len(heads) == len(tails)
    return [(200 * a, window_of(b, L)[1]) for a, b in zip(heads, tails)]


# ---- sequences -----------------------------------------------------------------------------------------------------------------------------
def background(rng, n):
    """n random bases without a telomere unit of either strand"""
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()
    while b"TTAGGG" in s or b"CCCTAA" in s:
        s = s.replace(b"TTAGGG", b"TTATGG").replace(b"CCCTAA", b"CCCCAA")
    return s


def telomere(n, unit=b"TTAGGG"):
    return (unit * (n // len(unit) + 1))[:n]


def planted(rng, L, blocks, unit=b"TTAGGG"):
    """a record of L bases: background with telomere repeats over every [a, b) of `blocks`"""
    s = bytearray(background(rng, L))
    for a, b in blocks:
        s[a:b] = telomere(b - a, unit)
    return bytes(s)


def random_assembly(rng, max_len=130_000):
    """1-6 records of 0 to max_len bases: telomere blocks of random lengths, some thinned by substitutions to densities around the threshold,
    more of them near the ends; the forward and the reverse unit"""
    recs = []
    for i in range(int(rng.integers(1, 7))):
        L = int(rng.choice([0, 1, 999, 1000, 1001, 51200, 51201])) if rng.random() < 0.15 else int(rng.integers(0, max_len + 1))
        s = bytearray(background(rng, L))
        for _ in range(int(rng.integers(0, 9))) if L > 0 else []:
            n = int(rng.choice([300, 500, 1000, 3000, 12000]))
            a = int(rng.choice([0, max(0, L - n)])) if rng.random() < 0.4 else int(rng.integers(0, L))
            b = min(L, a + n)
            blk = bytearray(telomere(b - a, b"TTAGGG" if rng.random() < 0.6 else b"CCCTAA"))
            if rng.random() < 0.5 and b > a:      # thinned: a substitution every few units
                for p in rng.integers(0, b - a, size=(b - a) // int(rng.integers(7, 40)) + 1):
                    blk[int(p)] = ord("A")
            s[a:b] = blk
        recs.append((b"ctg%d" % i, bytes(s)))
    return recs


def fasta(records, width=80):
    out = []
    for name, seq in records:
        out.append(b">" + name + b"\n")
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
def run_cli(cli, argv, cwd, env=None):
    e = dict(os.environ)
    for k in ("CORNETTO_ACCEL", "CORNETTO_DEVICE", "CORNETTO_DEVICES", "CORNETTO_CLI_WHOLE", "CORNETTO_FASTQ_PIECE", "CORNETTO_BATCH_BASES"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([cli] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=cwd)
    return {"rc": p.returncode, "out": p.stdout, "err": p.stderr}


def check_cli(cli, records, path, cwd, env=None, opts=(), m=b"TTAGGG", t="0.4", I="99.9", d=100, E=50000, exp=None):
    """`cornetto telostats <opts> path` in cwd under env: exit 0, stdout and the BED as expected(); opts must spell out what differs from
    the defaults.  -> (stdout, BED bytes)"""
    exp = exp or expected(records, m, float(t), float(I), d, E)
    bed = os.path.join(cwd, "out.bed")
    if os.path.exists(bed):
        os.remove(bed)
    got = run_cli(cli, ["telostats"] + list(opts) + ["-b", bed, path], cwd, env)
    assert got["rc"] == 0, got["err"][-2000:]
    assert got["out"] == stdout_text(path, exp, t, d, E), (got["out"], got["err"][-1500:])
    with open(bed, "rb") as f:
        text = f.read()
    assert text == bed_text(records, exp), (text[-600:], bed_text(records, exp)[-600:])
    return got["out"], text
