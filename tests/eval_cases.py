"""Shared by tests/test_eval_host.py, tests/test_gpu_eval.py and tests/golden/make_golden_eval.py: the fixture inputs and recorded cases of
the evaluation sub-commands `cornetto nx | report | telocontigs | asmstats`, a runner that returns stdout bytes and the exit status, a Python
restatement of what the reference prints (src/nx.c, src/report.c, src/telocontigs.c, src/asmstats.c), and seeded random cases."""
import functools
import gzip
import json
import os
import random
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
EVAL = os.path.join(GOLDEN, "eval")
REF_CLI = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "cornetto")


# ---- fixture inputs ---------------------------------------------------------------------------------------------------------------------
def fasta_text(recs, width=60, rng=None):
    """records (name, length[, comment]) -> FASTA text; lines wrapped at `width` (random widths and blank lines with rng)"""
    out = []
    for i, r in enumerate(recs):
        name, n = r[0], r[1]
        out.append(">%s%s\n" % (name, (" " + r[2]) if len(r) > 2 else ""))
        seq = "".join("ACGTNacgt"[(i * 7 + k * 13) % 9] for k in range(n)) if not rng else "".join(rng.choice("ACGTN") for _ in range(n))
        w = rng.choice([5, 60, 61, 1000]) if rng else width
        for k in range(0, n, w):
            out.append(seq[k:k + w] + "\n")
        if rng and rng.random() < 0.2:
            out.append("\n")
    return "".join(out)


def fastq_text(recs):
    return "".join("@%s extra\n%s\n+\n%s\n" % (name, "ACGT" * (n // 4) + "A" * (n % 4), "I" * n) for name, n in recs)


# the assembly fixture: ties in length (kept in input order by telocontigs), an empty record, a comment, wrapped lines
ASM = [("ctgA", 500), ("ctgB", 120, "len=120"), ("ctgC", 500), ("ctgD", 0), ("ctgE", 77), ("ctgF", 1200), ("ctgG", 120), ("ctgH", 3)]
READS = [("r%d" % i, (i * 37) % 90 + 1) for i in range(40)]
# a FASTA with a FASTQ record in the middle: plain at first, the rest is the sequential reader's
MIXED = fasta_text(ASM[:3]) + "@q1\nACGTACGT\n+\nIIIIIIII\n" + fasta_text(ASM[3:])
# 250 records: the reference's contig array moves at 100 and 200 records; rows only on records >= 200 keep its output defined
MANY = [("m%03d" % i, (i * 7919) % 500 + 1) for i in range(250)]

TEL_BED = "ctgA\t0\t100\nctgA\t400\t500\nctgC\t0\t10\nctgF\t5\t60\nctgF\t70 80\nctgF\t1100\t1200\nctgH\t0\t3\n"
MANY_BED = "".join("m%03d\t0\t1\n" % i for i in (200, 201, 249, 249, 230))

# asmstats: contigs of the report on chromosomes of a small reference; names that compare equal in natural order (chr1 / chr01)
AS_BED = "ctgA\t0\t100\nctgA\t400\t500\nctgC\t0\t10\nctgT\t0\t5\nctgF\t1100\t1200\nctgX\t3\t9\nctgX\t10\t20\nctgX\t30\t40\n"
AS_REPORT = ("ctgA\tchr1\t+\t1\nctgB\tchr2\t-\nctgC\tchr1\nctgF\tchr10\tx\ty\nctgG\tchr01\nctgH\tchrX\nctgX\tchr2\nctgB\tchr1\n"
             "ctgZ\tchr3\n")
AS_PAF = ("ctgA\t500\t0\t400\t+\tchr1\t200000\t0\t150000\t400\t400\t60\n"
          "ctgA\t500\t400\t500\t+\tchr2\t300000\t10\t20\t10\t10\t60\n"
          "ctgB\t120\t0\t120\t-\tchr1\t200000\t150000\t160000\t120\t120\t60\n"
          "ctgB\t120\t0\t120\t-\tchr2\t300000\t0\t1200000\t120\t120\t60\n"
          "ctgC\t500\t0\t500\t+\tchr1\t200000\t0\t50000\t500\t500\t1\n"
          "ctgF\t1200\t0\t1200\t+\tchr10\t900000\t0\t600000\t1200\t1200\t60\n"
          "ctgG\t120\t0\t120\t+\tchr01\t5000\t100\t100\t120\t120\t60\n"
          "ctgH\t3\t0\t3\t+\tchrX\t7000\t0\t3\t3\t3\t60\n"
          "ctgX\t800\t0\t800\t+\tchr2\t300000\t0\t20000000\t800\t800\t60\n"
          "ctgX\t800\t0\t800\t+\tchr1\t200000\t5\t4\t800\t800\t60\n"
          "ctgQ\t50\t0\t50\t+\tchr1\t200000\t0\t50\t50\t50\t60\n"
          "ctgZ\t9\t0\t9\t+\tchr3_PATERNAL\t400\t0\t9\t9\t9\t60\n"
          "ctgZ\t9\t0\t9\t+\tchr3\t400\t0\t200\t9\t9\t60\n")
REF_FA = fasta_text([("chr2", 5), ("chrX", 3), ("chr1", 4), ("chrM", 2), ("chr01", 1), ("chr10", 6), ("chr3", 1)])


def golden_inputs(d):
    """write the fixture inputs into directory d -> dict of paths"""
    p = {}
    texts = {
        "asm.fa": fasta_text(ASM), "reads.fq": fastq_text(READS), "mixed.fa": MIXED, "many.fa": fasta_text(MANY, 70),
        "empty.fa": "", "allempty.fa": ">e1\n>e2 x\n", "dup.fa": fasta_text([("d1", 5), ("d2", 9), ("d1", 3)]),
        "tel.bed": TEL_BED, "many.bed": MANY_BED, "empty.bed": "",
        "bed_header.bed": "track name=x\nctgA\t0\t10\n", "bed_blank.bed": "ctgA\t0\t10\n\n", "bed_neg.bed": "ctgA\t-1\t10\n",
        "bed_startend.bed": "ctgA\t10\t10\n", "bed_two.bed": "ctgA\t10\n", "bed_unknown.bed": "ctgA\t0\t10\nnope\t0\t10\n",
        "bed_backwards.bed": "ctgA\t10\t5\n",
        "as.bed": AS_BED, "as.report.tsv": AS_REPORT, "as.paf": AS_PAF, "ref.fa": REF_FA,
        "report_onefield.tsv": "ctgA\tchr1\nctgB\n", "report_nopaf.tsv": AS_REPORT + "ctgA\tchr9\n",
        "paf_qlen.paf": AS_PAF + "ctgA\t501\t0\t1\t+\tchr1\t200000\t0\t1\t1\t1\t60\n",
        "paf_tlen.paf": AS_PAF + "ctgB\t120\t0\t1\t+\tchr1\t200001\t0\t1\t1\t1\t60\n",
        "paf_short.paf": AS_PAF + "ctgA\t500\t0\t1\t+\tchr1\t200000\t0\t1\t1\t1\n",
    }
    for name, text in texts.items():
        f = os.path.join(d, name)
        with open(f, "w", newline="") as fh:
            fh.write(text)
        p[name] = f
    for name in ("asm.fa", "reads.fq", "mixed.fa"):
        f = os.path.join(d, name + ".gz")
        with open(f, "wb") as fh:
            fh.write(gzip.compress(texts[name].encode(), 6, mtime=0))
        p[name + ".gz"] = f
    return p


# recorded cases: (case id, argv with input names)
_AS = ["as.paf", "as.bed", "-r", "as.report.tsv"]
GOLDEN_CASES = [
    ("nx_asm", ["nx", "asm.fa"]),
    ("nx_gz", ["nx", "asm.fa.gz"]),
    ("nx_fastq", ["nx", "reads.fq"]),
    ("nx_fastq_gz", ["nx", "reads.fq.gz"]),
    ("nx_mixed", ["nx", "mixed.fa"]),
    ("nx_g", ["nx", "-g", "3.1k", "asm.fa"]),
    ("nx_g_long", ["nx", "--genome-size=2.5K", "asm.fa"]),
    ("nx_g_m", ["nx", "asm.fa", "-g", "0.000004m"]),
    ("nx_g_round", ["nx", "-g", "1000.5", "asm.fa"]),
    ("nx_g_zero", ["nx", "-g", "0", "asm.fa"]),
    ("nx_g_neg", ["nx", "-g", "-5G", "asm.fa"]),
    ("nx_g_text", ["nx", "-g", "abc", "nonexistent.fa"]),
    ("nx_allempty", ["nx", "allempty.fa"]),
    ("nx_empty", ["nx", "empty.fa"]),
    ("nx_missing", ["nx", "nonexistent.fa"]),
    ("nx_help", ["nx", "-h"]),
    ("nx_help_file", ["nx", "asm.fa", "--help"]),
    ("nx_no_args", ["nx"]),
    ("nx_two_args", ["nx", "asm.fa", "asm.fa"]),
    ("report_one", ["report", "asm.fa"]),
    ("report_many", ["report", "asm.fa", "asm.fa.gz", "reads.fq", "reads.fq.gz", "mixed.fa", "mixed.fa.gz", "allempty.fa", "empty.fa", "many.fa"]),
    ("report_missing", ["report", "asm.fa", "nonexistent.fa", "reads.fq"]),
    ("report_help_late", ["report", "asm.fa", "-h"]),
    ("report_no_args", ["report"]),
    ("report_verbose", ["report", "--verbose", "2", "asm.fa"]),
    ("telo_asm", ["telocontigs", "asm.fa", "tel.bed"]),
    ("telo_gz", ["telocontigs", "asm.fa.gz", "tel.bed"]),
    ("telo_mixed", ["telocontigs", "mixed.fa", "tel.bed"]),
    ("telo_fastq", ["telocontigs", "reads.fq", "empty.bed"]),
    ("telo_many", ["telocontigs", "many.fa", "many.bed"]),
    ("telo_dup", ["telocontigs", "dup.fa", "empty.bed"]),
    ("telo_header", ["telocontigs", "asm.fa", "bed_header.bed"]),
    ("telo_blank", ["telocontigs", "asm.fa", "bed_blank.bed"]),
    ("telo_neg", ["telocontigs", "asm.fa", "bed_neg.bed"]),
    ("telo_startend", ["telocontigs", "asm.fa", "bed_startend.bed"]),
    ("telo_backwards", ["telocontigs", "asm.fa", "bed_backwards.bed"]),
    ("telo_two_fields", ["telocontigs", "asm.fa", "bed_two.bed"]),
    ("telo_unknown", ["telocontigs", "asm.fa", "bed_unknown.bed"]),
    ("telo_missing_fa", ["telocontigs", "nonexistent.fa", "tel.bed"]),
    ("telo_missing_bed", ["telocontigs", "asm.fa", "nonexistent.bed"]),
    ("telo_help", ["telocontigs", "-h", "asm.fa", "tel.bed"]),
    ("telo_one_arg", ["telocontigs", "asm.fa"]),
    ("as_default", ["asmstats"] + _AS),
    ("as_human1", ["asmstats", "-s", "human1"] + _AS),
    ("as_human2", ["asmstats", "--sort-order", "human2"] + _AS),
    ("as_ref", ["asmstats", "-s", "ref.fa"] + _AS),
    ("as_ref_gz", ["asmstats", "-s", "asm.fa.gz"] + _AS),
    ("as_ref_fastq", ["asmstats", "-s", "reads.fq"] + _AS),
    ("as_ref_mixed", ["asmstats", "-s", "mixed.fa"] + _AS),
    ("as_ref_missing", ["asmstats", "-s", "nonexistent.fa"] + _AS),
    ("as_trim", ["asmstats", "--trim-pat-mat"] + _AS),
    ("as_trim_prefix", ["asmstats", "--tr", "-s", "ref.fa"] + _AS),
    ("as_report_long", ["asmstats", "--report=" + "as.report.tsv", "as.paf", "as.bed"]),
    ("as_no_report", ["asmstats", "as.paf", "as.bed"]),
    ("as_help", ["asmstats", "-h"]),
    ("as_help_full", ["asmstats", "-h"] + _AS),
    ("as_one_arg", ["asmstats", "-r", "as.report.tsv", "as.paf"]),
    ("as_empty_bed", ["asmstats", "as.paf", "empty.bed", "-r", "as.report.tsv"]),
    ("as_bed_bad", ["asmstats", "as.paf", "bed_neg.bed", "-r", "as.report.tsv"]),
    ("as_bed_blank", ["asmstats", "as.paf", "bed_blank.bed", "-r", "as.report.tsv"]),
    ("as_report_onefield", ["asmstats", "as.paf", "as.bed", "-r", "report_onefield.tsv"]),
    ("as_report_nopaf", ["asmstats", "as.paf", "as.bed", "-r", "report_nopaf.tsv"]),
    ("as_report_nopaf_h1", ["asmstats", "-s", "human1", "as.paf", "as.bed", "-r", "report_nopaf.tsv"]),
    ("as_paf_qlen", ["asmstats", "paf_qlen.paf", "as.bed", "-r", "as.report.tsv"]),
    ("as_paf_tlen", ["asmstats", "paf_tlen.paf", "as.bed", "-r", "as.report.tsv"]),
    ("as_paf_short", ["asmstats", "paf_short.paf", "as.bed", "-r", "as.report.tsv"]),
    ("as_missing_paf", ["asmstats", "nonexistent.paf", "as.bed", "-r", "as.report.tsv"]),
    ("as_missing_report", ["asmstats", "as.paf", "as.bed", "-r", "nonexistent.tsv"]),
]


def run_case(cli, argv, inputs, d, env=None):
    """one invocation -> dict(rc, out, err); input names are resolved through `inputs`"""
    a = [inputs.get(x, x) if not x.startswith("--") or "=" not in x else x.split("=", 1)[0] + "=" + inputs.get(x.split("=", 1)[1], x.split("=", 1)[1])
         for x in argv]
    e = dict(os.environ)
    e.pop("CORNETTO_ACCEL", None)
    e.update(env or {})
    p = subprocess.run([cli] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=d)
    return {"rc": p.returncode, "out": p.stdout, "err": p.stderr}


def portable(out, inputs):
    """stdout with the fixture directory taken out (report and asmstats print the paths they were given)"""
    for name, path in sorted(inputs.items(), key=lambda kv: -len(kv[1])):
        out = out.replace(path.encode(), b"<" + name.encode() + b">")
    return out


def load_golden(case):
    exp = json.load(open(os.path.join(EVAL, case + ".json")))
    return {"rc": exp["rc"], "out": exp["out"].encode("latin-1")}


def same(got, exp, inputs):
    g = {"rc": got["rc"], "out": portable(got["out"], inputs)}
    e = {"rc": exp["rc"], "out": portable(exp["out"], inputs)}
    assert g == e, (g["rc"], e["rc"], g["out"][-600:], e["out"][-600:], got.get("err", b"")[-1500:])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def _cf(x):
    """C's "%f" (x86 prints the NaN of 0.0 / 0.0 as -nan)"""
    return "-nan" if x != x else "%f" % x


def nx_text(lens, genome=None):
    out = ["#x\tcontig_len\n"]
    s, cum, pct = sum(lens), 0, 0.0
    for n in sorted(lens, reverse=True):
        out.append("%s\t%d\n" % (_cf(pct), n))
        cum += n
        if genome:
            pct = cum / genome * 100
        else:
            pct = cum / s * 100 if s else float("nan")
        out.append("%s\t%d\n" % (_cf(pct), n))
    return "".join(out).encode()


def parse_num(s):
    """mm_parse_num (src/misc.c:72-84) for the plain decimal forms the random cases use"""
    m = re.match(r"\s*([+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?)", s)
    x = float(m.group(1)) if m else 0.0
    rest = s[m.end():] if m else s
    mul = {"G": 1e9, "g": 1e9, "M": 1e6, "m": 1e6, "K": 1e3, "k": 1e3}.get(rest[:1], 1.0)
    if rest[:1] in "GgMmKk" and rest[:1]:
        x *= mul
    return int(x + .499) if x + .499 >= 0 else -int(-(x + .499))


def report_row(lens):
    if not lens:
        return "0\t0.001\t0.000\t0.000\n"       # the reference prints the heap chunk header of its empty array (0x331 = 817) as the longest
    s, cum, n50, n90 = sum(lens), 0, 0, 0
    for n in sorted(lens, reverse=True):
        cum += n
        if cum >= s * 0.5 and n50 == 0:
            n50 = n
        if cum >= s * 0.9 and n90 == 0:
            n90 = n
    return "%d\t%.3f\t%.3f\t%.3f\n" % (len(lens), max(lens) / 1e6, n50 / 1e6, n90 / 1e6)


def report_text(paths, lens_of):
    return ("#asm\tNcontigs\tLargestcontig(Mbase)\tN50(Mbase)\tN90(Mbase)\n" + "".join(p + "\t" + report_row(lens_of[p]) for p in paths)).encode()


def _lines(text):
    """the lines getline() returns, without their newline"""
    b = text.encode()
    return [] if not b else (b[:-1] if b.endswith(b"\n") else b).split(b"\n")


def bed_rows(text):
    """the contig of every row of a telomere BED, or None where the reference exits 1"""
    rows = []
    for line in _lines(text):
        t = line.split()
        if len(t) < 3 or not re.fullmatch(rb"[+-]?\d+", t[1]) or not re.fullmatch(rb"[+-]?\d+", t[2]):
            return None
        b, e = int(t[1]), int(t[2])
        if e < b or b < 0 or e < 0 or b >= e:
            return None
        rows.append(t[0].decode())
    return rows


def telocontigs_text(recs, bed):
    """recs: [(name, length)] -> (rc, stdout); the counts the program means (see the header of cornetto_amd/cli/eval_main.c)"""
    names = [r[0] for r in recs]
    if len(set(names)) != len(names):
        return 1, b""
    rows = bed_rows(bed)
    if rows is None or any(r not in names for r in rows):
        return 1, b""
    nt = {n: 0 for n in names}
    for r in rows:
        nt[r] += 1
    order = sorted(range(len(recs)), key=lambda i: -recs[i][1])
    return 0, ("Contig\tLength\tNTelomeres\n" + "".join("%s\t%d\t%d\n" % (recs[i][0], recs[i][1], nt[recs[i][0]]) for i in order)).encode()


def strnum_cmp(a, b):
    """src/misc.c:139-171 on byte strings"""
    dig = lambda c: 48 <= c <= 57  # noqa: E731
    i = j = 0
    while i < len(a) and j < len(b):
        if not dig(a[i]) or not dig(b[j]):
            if a[i] != b[j]:
                return a[i] - b[j]
            i += 1
            j += 1
            continue
        while i < len(a) and a[i] == 48:
            i += 1
        while j < len(b) and b[j] == 48:
            j += 1
        while i < len(a) and j < len(b) and dig(a[i]) and a[i] == b[j]:
            i += 1
            j += 1
        ca = a[i] if i < len(a) else 0
        cb = b[j] if j < len(b) else 0
        diff = ca - cb
        while i < len(a) and j < len(b) and dig(a[i]) and dig(b[j]):
            i += 1
            j += 1
        if i < len(a) and dig(a[i]):
            return 1
        if j < len(b) and dig(b[j]):
            return -1
        if diff:
            return diff
    return 1 if i < len(a) else (-1 if j < len(b) else 0)


def _atoi(s):
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?\d+)", s)
    v = int(m.group(1)) if m else 0
    v = max(min(v, (1 << 63) - 1), -(1 << 63)) & 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


HUMAN1 = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"]
HUMAN2 = [x for k in range(1, 23) for x in ("chr%d_MATERNAL" % k, "chr%d_PATERNAL" % k)] + ["chrX_MATERNAL", "chrY_PATERNAL"]


def asmstats_text(paf_arg, bed, report, paf, order=None, trim=False, ref_names=None, kh=None):
    """(rc, stdout) of `asmstats paf_arg <bed> -r <report> [-s order] [--trim-pat-mat]`; texts of the three files; ref_names: the record
    names of the -s FASTA; kh: cornetto_amd.khash_str_order"""
    rows = bed_rows(bed)
    if rows is None:
        return 1, b""
    ctg, ckeys = {}, []

    def put(n):
        if n not in ctg:
            ctg[n] = {"ntelo": 0, "len": 0, "chr": None, "recs": []}
            ckeys.append(n)
        return ctg[n]
    for r in rows:
        put(r)["ntelo"] += 1
    chr_len, hkeys = {}, []
    for line in _lines(report):
        t = line.split()
        if len(t) < 2:
            return 1, b""
        put(t[0].decode())["chr"] = t[1].decode()
        if t[1].decode() not in chr_len:
            chr_len[t[1].decode()] = 0
            hkeys.append(t[1].decode())
    for line in _lines(paf):
        f = [x for x in re.split(rb"[\t\r\n]", line) if x]
        if len(f) < 12:
            return 1, b""
        rid, tid = f[0].decode(), f[5].decode()
        if trim:
            tid = tid.split("_PATERNAL", 1)[0].split("_MATERNAL", 1)[0]
        if rid not in ctg:
            continue
        c = ctg[rid]
        q = _atoi(f[1]) & 0xFFFFFFFF
        if c["len"] == 0:
            c["len"] = q
        elif c["len"] != q:
            return 1, b""
        c["recs"].append((tid, (_atoi(f[8]) - _atoi(f[7])) & 0xFFFFFFFF))
        if tid in chr_len:
            tl = _atoi(f[6]) & 0xFFFFFFFF
            if chr_len[tid] == 0:
                chr_len[tid] = tl
            elif chr_len[tid] != tl:
                return 1, b""
    if order is None:
        lst = [hkeys[i] for i in kh([k.encode() for k in hkeys])[1]] if hkeys else []
        lst = sorted(lst, key=functools.cmp_to_key(lambda a, b: strnum_cmp(a.encode(), b.encode())))
    elif order == "human1":
        lst = HUMAN1
    elif order == "human2":
        lst = HUMAN2
    else:
        if ref_names is None:
            return 1, b""
        lst = ref_names
    corder = [ckeys[i] for i in kh([k.encode() for k in ckeys])[1]] if ckeys else []
    out = [paf_arg + "\n\n", "chr\tT2T?\tNTelo\tTelocontiglen\n"]
    for ch in lst:
        sel = [ctg[k] for k in corder if ctg[k]["chr"] == ch and ctg[k]["ntelo"] > 0]
        if sel:
            out.append("%s\t%s\t%d\t%s\n" % (ch, "".join("y," if c["ntelo"] == 2 else "n," for c in sel), sum(c["ntelo"] for c in sel),
                                             "".join("%d," % (c["len"] - (1 << 32) if c["len"] >> 31 else c["len"]) for c in sel)))
        else:
            out.append("%s\t\t\t\n" % ch)
    hdr = "\tNcontigsofsize>=KMbasealignedtochr\t\t\t\t\t%ofchrsequencecoveredbycontigsofsize>=KMbase\n" \
          "chr\t0Mbase\t0.1Mbase\t1Mbase\t5Mbase\t10Mbase\t0Mbase\t0.1Mbase\t1Mbase\t5Mbase\t10Mbase\n"
    titles = ["Contigs whose majority is mapped to the corresponding chromosome\n" + hdr,
              "LX of Contigs whose majority is mapped to the corresponding chromosome\n\tL50\tL90\tL95\tL99\tCumCovN5\n",
              "Contigs whose majority is mapped to another chromosome\n" + hdr]
    for table in range(3):
        out.append("\n\n" + titles[table])
        for ch in lst:
            if ch not in chr_len:
                out.append(ch + "\n")
                continue
            L = chr_len[ch]
            if L == 0:
                return 1, "".join(out).encode()
            if table != 1:
                cnt, sm = [0] * 5, [0] * 5
                for c in ctg.values():
                    if c["chr"] is None or (c["chr"] == ch) != (table == 0) or not c["recs"]:
                        continue
                    ta = sum(a for t, a in c["recs"] if t == ch)
                    for b, lim in enumerate((1, 100000, 1000000, 5000000, 10000000)):
                        if ta >= lim:
                            cnt[b] += 1
                            sm[b] += ta
                out.append("%s\t%s\t%s\n" % (ch, "\t".join(str(x) for x in cnt), "\t".join("%.3f" % (s / L * 100) for s in sm)))
            else:
                aln = sorted((sum(a for t, a in c["recs"] if t == ch) & 0xFFFFFFFF for c in ctg.values() if c["chr"] == ch and c["recs"]),
                             reverse=True)
                lx, s, cov = [0] * 4, 0, [0] * 5
                for q, a in enumerate(aln):
                    s += a
                    for f, fr in enumerate((0.50, 0.90, 0.95, 0.99)):
                        if s >= L * fr and lx[f] == 0:
                            lx[f] = q + 1
                    for f in range(q, 5):
                        cov[f] += a
                out.append("%s\t%s\t%s\n" % (ch, "\t".join(str(x) for x in lx), ",".join("%.3f" % (v / L * 100) for v in cov)))
    return 0, "".join(out).encode()


# ---- seeded random cases ------------------------------------------------------------------------------------------------------------------
def _write(d, name, text, gz=False):
    f = os.path.join(d, name + (".gz" if gz else ""))
    with open(f, "wb") as fh:
        fh.write(gzip.compress(text.encode(), 6, mtime=0) if gz else text.encode())
    return f


def _rand_recs(rng, n_max=30, dup=False):
    n = rng.randrange(0, n_max)
    names = ["s%d" % rng.randrange(1000 if not dup else 5) for _ in range(n)]
    if not dup:
        seen, uniq = set(), []
        for x in names:
            if x not in seen:
                seen.add(x)
                uniq.append(x)
        names = uniq
    return [(x, rng.choice([0, 1, 5, 50, 200, 200, 1000]) if rng.random() < 0.5 else rng.randrange(0, 3000)) for x in names]


def random_case(kind, seed, d, kh):
    """-> (argv with paths, expected (rc, stdout))"""
    rng = random.Random(seed)
    if kind == "nx":
        recs = _rand_recs(rng)
        f = _write(d, "r.fa", fasta_text(recs, rng=rng), gz=rng.random() < 0.3)
        g = rng.choice([None, None, "1000", "2.5k", "0.001M", "7e3"])
        return (["nx"] + (["-g", g] if g else []) + [f]), (0, nx_text([r[1] for r in recs], parse_num(g) if g else None))
    if kind == "report":
        paths, lens_of = [], {}
        for k in range(rng.randrange(1, 5)):
            recs = _rand_recs(rng)
            f = _write(d, "r%d.fa" % k, fasta_text(recs, rng=rng), gz=rng.random() < 0.3)
            paths.append(f)
            lens_of[f] = [r[1] for r in recs]
        return ["report"] + paths, (0, report_text(paths, lens_of))
    if kind == "telocontigs":
        recs = _rand_recs(rng, 60, dup=rng.random() < 0.1)[:100]        # (<= 100 records: where the reference's counts are defined)
        rows = []
        for _ in range(rng.randrange(0, 12)):
            nm = rng.choice([r[0] for r in recs]) if recs and rng.random() < 0.95 else "nope"
            b = rng.randrange(0, 50)
            e = b + rng.randrange(1, 20) if rng.random() < 0.97 else b
            rows.append("%s\t%d\t%d\n" % (nm, b, e))
        fa = _write(d, "t.fa", fasta_text(recs, rng=rng), gz=rng.random() < 0.3)
        bed = _write(d, "t.bed", "".join(rows))
        return ["telocontigs", fa, bed], telocontigs_text(recs, "".join(rows))
    # asmstats
    chrs = rng.sample(["chr1", "chr01", "chr2", "chr10", "chrX", "chr1_PATERNAL", "chr2_MATERNAL", "chrM", "a9", "a09b"], rng.randrange(1, 7))
    ctgs = ["c%d" % i for i in range(rng.randrange(1, 25))]
    bed = "".join("%s\t%d\t%d\n" % (rng.choice(ctgs + ["u1"]), 0, rng.randrange(1, 9)) for _ in range(rng.randrange(0, 20)))
    report = "".join("%s\t%s%s\n" % (c, rng.choice(chrs), "\textra" if rng.random() < 0.2 else "") for c in ctgs if rng.random() < 0.8)
    qlen = {c: rng.choice([0, 100, 5000, 2000000]) for c in ctgs + ["u2"]}
    tlen = {t: rng.choice([1000000, 30000000, 250000000]) for t in chrs}
    lines = []
    for _ in range(rng.randrange(0, 40)):
        c = rng.choice(ctgs + ["u2"])
        t = rng.choice(chrs)
        ts = rng.randrange(0, 1000)
        te = ts + rng.choice([0, 1, 99999, 100000, 1000000, 5000001, 12000000, rng.randrange(0, 3000000)])
        ql = qlen[c] if rng.random() < 0.98 else qlen[c] + 1
        lines.append("%s\t%d\t0\t10\t+\t%s\t%d\t%d\t%d\t10\t10\t60\n" % (c, ql, t, tlen[t], ts, te))
    # every report chromosome gets one PAF line most of the time (else the program ends in table 2)
    for t in chrs:
        if rng.random() < 0.9 and ctgs:
            lines.append("%s\t%d\t0\t10\t-\t%s\t%d\t0\t5\t10\t10\t60\n" % (ctgs[0], qlen[ctgs[0]], t, tlen[t]))
    rng.shuffle(lines)
    paf = "".join(lines)
    order = rng.choice([None, None, "human1", "ref"])
    trim = rng.random() < 0.2
    fb, fr, fp = _write(d, "a.bed", bed), _write(d, "a.tsv", report), _write(d, "a.paf", paf)
    argv = ["asmstats", fp, fb, "-r", fr] + (["--trim-pat-mat"] if trim else []) + (["-s", "human1"] if order == "human1" else [])
    ref_names = None
    if order == "ref":
        ref_names = rng.sample(chrs + ["chrQ"], rng.randrange(0, len(chrs) + 1))
        argv += ["-s", _write(d, "ref.fa", fasta_text([(x, rng.randrange(0, 9)) for x in ref_names], rng=rng), gz=rng.random() < 0.3)]
    return argv, asmstats_text(fp, bed, report, paf, order if order != "ref" else "file", trim, ref_names, kh)


def check_random(cli, kind, seed, d, env=None, kh=None):
    argv, (rc, out) = random_case(kind, seed, d, kh)
    got = run_case(cli, argv, {}, d, env)
    assert (got["rc"], got["out"]) == (rc, out), (kind, seed, argv, got["rc"], rc, got["out"][-800:], out[-800:], got["err"][-1500:])
    if os.path.exists(REF_CLI):
        ref = run_case(REF_CLI, argv, {}, d)
        assert (ref["rc"], ref["out"]) == (rc, out), ("reference", kind, seed, argv, ref["rc"], ref["out"][-800:], out[-800:])
