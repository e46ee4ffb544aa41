"""Shared by tests/test_fixasm_host.py, tests/test_gpu_fixasm.py and tests/golden/make_golden_fixasm.py: the recorded `cornetto fixasm`
cases, a Python restatement of what the reference prints (src/fixasm.c:226-405, src/pafrec.c:43-98) for records given as lists, a seeded
random case generator, and a runner that collects every output of one invocation."""
import gzip
import json
import os
import random
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIX = os.path.join(GOLDEN, "fixasm")
REF_CLI = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "cornetto")

# the PAF fixture: every quirk of the list in the module docstring of cornetto_amd/cli/fixasm_main.c
#   ctgA  + and - bases tie (stays +), two targets tie in lines (the later one, chr2, wins), tp:A:S, runs of tabs
#   ctgB  mostly - (reversed), mapq 300 (prints 44), an unknown strand '*' counts as '-', CRLF
#   ctgC  the empty record, on chr1_PATERNAL; ctgD on chr1_MATERNAL (both chr1_0 under --trim-pat-mat)
#   ctgJ  lower case, reversed: lower case is reversed but not complemented
#   ctgZ  only in the PAF: "(null)" in -w.  ctgE..ctgI are not in the PAF: dropped, listed by -m
MIX_PAF = (
    "ctgA\t5000\t0\t100\t+\tchr1_PATERNAL\t100000\t10\t60\t50\t50\t60\ttp:A:S\n"
    "ctgA\t5000\t100\t200\t-\tchr2\t200000\t500\t550\t40\t50\t60\n"
    "ctgA\t5000\t\t\t200\t300\t+\tchr2\t200000\t700\t700\t40\t50\t0\tcg:Z:5M\n"
    "ctgA\t5000\t300\t400\t+\tchr1_PATERNAL\t100000\t0\t0\t1\t1\t1\ttp:A:P\n"
    "ctgB\t64\t0\t64\t-\tchr2\t200000\t0\t64\t64\t64\t300\ttp:A:S\r\n"
    "ctgB\t64\t1\t2\t*\tchr2\t200000\t100\t101\t1\t1\t7\r\n"
    "ctgB\t64\t3\t9\t+\tchrX\t9000\t5\t10\t5\t5\t255\n"
    "ctgC\t0\t0\t0\t+\tchr1_PATERNAL\t100000\t1\t2\t1\t1\t0\n"
    "ctgD\t63\t0\t63\t+\tchr1_MATERNAL\t100000\t0\t63\t63\t63\t60\ttp:A:Q\n"
    "ctgJ\t2\t0\t2\t-\tchr1_PATERNAL\t100000\t0\t2\t2\t2\t-5\n"
    "ctgZ\t10\t0\t10\t-\tchrX\t9000\t0\t10\t10\t10\t1\n"
)
# a FASTA with a name given twice (renamed twice; -w takes the last name) and an IUPAC / N mix
DUP_FA = ">d1 x\nACGTNRYKMacgtn\n>d2\nAAAA\nCCCC\n>d1\nGGGTTT\n>d3\nTTTT\n"
DUP_PAF = ("d1\t14\t0\t14\t-\tchrM\t16000\t0\t10\t9\t10\t60\n"
           "d2\t8\t0\t8\t+\tchrM\t16000\t0\t8\t8\t8\t60\n"
           "d3\t4\t0\t4\t-\tchrM\t16000\t0\t4\t4\t4\t60\n"
           "d3\t4\t0\t4\t+\tchrM\t16000\t0\t4\t4\t4\t60\n")


def golden_inputs(d):
    """write the fixture inputs into directory d -> dict of paths"""
    p = {"mix.fa.gz": os.path.join(GOLDEN, "mix.fa.gz")}
    for name, text in (("mix.paf", MIX_PAF), ("dup.fa", DUP_FA), ("dup.paf", DUP_PAF),
                       ("blank.paf", MIX_PAF.split("\n", 1)[0] + "\n\n"), ("short.paf", "ctgA\t1\t2\t3\t+\tchr\t1\t2\t3\t4\t5\n"),
                       ("empty.paf", "")):
        f = os.path.join(d, name)
        with open(f, "w", newline="") as fh:
            fh.write(text)
        p[name] = f
    return p


# recorded cases: (case id, argv with input names and {R} {M} {W} for the output files)
GOLDEN_CASES = [
    ("mix", ["fixasm", "-r", "{R}", "-m", "{M}", "-w", "{W}", "mix.fa.gz", "mix.paf"]),
    ("mix_trim", ["fixasm", "--trim-pat-mat", "-r", "{R}", "-m", "{M}", "-w", "{W}", "mix.fa.gz", "mix.paf"]),
    ("mix_long", ["fixasm", "--report={R}", "--missing", "{M}", "--tr", "-w", "{W}", "mix.fa.gz", "mix.paf"]),
    ("mix_prefix", ["fixasm", "--rep", "{R}", "--mis={M}", "-x", "mix.fa.gz", "-v", "1", "mix.paf"]),
    ("mix_plain", ["fixasm", "mix.fa.gz", "mix.paf"]),
    ("dup", ["fixasm", "-r", "{R}", "-m", "{M}", "-w", "{W}", "dup.fa", "dup.paf"]),
    ("empty_paf", ["fixasm", "-r", "{R}", "-m", "{M}", "-w", "{W}", "dup.fa", "empty.paf"]),
    ("help_two", ["fixasm", "-h", "-r", "{R}", "dup.fa", "dup.paf"]),
    ("help_one", ["fixasm", "-h", "dup.fa"]),
    ("no_args", ["fixasm"]),
    ("three_args", ["fixasm", "dup.fa", "dup.paf", "dup.paf"]),
    ("blank_line", ["fixasm", "-r", "{R}", "dup.fa", "blank.paf"]),
    ("eleven_fields", ["fixasm", "-r", "{R}", "dup.fa", "short.paf"]),
    ("missing_fasta", ["fixasm", "-r", "{R}", "nonexistent.fa", "dup.paf"]),
    ("missing_paf", ["fixasm", "dup.fa", "nonexistent.paf"]),
    ("bad_report", ["fixasm", "-r", "/nonexistent/dir/r.tsv", "dup.fa", "dup.paf"]),
    ("bad_wpaf", ["fixasm", "-r", "{R}", "-w", "/nonexistent/dir/w.paf", "dup.fa", "dup.paf"]),
]


def summary(err):
    """the three count lines fix_the_assembly() prints on stderr (:396)"""
    return [ln for ln in err.decode(errors="replace").splitlines() if ln.split(":")[0] in ("total", "negative", "missing")]


def run_case(cli, argv, inputs, d, env=None):
    """one invocation -> dict(rc, out, summary, report, missing, wpaf); input names are resolved through `inputs`"""
    files = {"{R}": os.path.join(d, "r.tsv"), "{M}": os.path.join(d, "m.txt"), "{W}": os.path.join(d, "w.paf")}
    for f in files.values():
        if os.path.exists(f):
            os.remove(f)
    a = []
    for x in argv:
        for k, v in files.items():
            x = x.replace(k, v)
        a.append(inputs.get(x, x))
    e = dict(os.environ)
    e.pop("CORNETTO_ACCEL", None)
    e.update(env or {})
    p = subprocess.run([cli] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=d)

    def rd(k):
        return open(files[k], "rb").read().decode("latin-1") if os.path.exists(files[k]) else None
    return {"rc": p.returncode, "out": p.stdout, "summary": summary(p.stderr), "report": rd("{R}"), "missing": rd("{M}"), "wpaf": rd("{W}"),
            "err": p.stderr}


def load_golden(case):
    exp = json.load(open(os.path.join(FIX, case + ".json")))
    exp["out"] = gzip.open(os.path.join(FIX, exp["out_file"])).read()
    return exp


def same(got, exp):
    for k in ("rc", "out", "summary", "report", "missing", "wpaf"):
        assert got[k] == exp[k], (k, got[k] if k != "out" else got[k][:400], exp[k] if k != "out" else exp[k][:400], got["err"][-2000:])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _atoi(s):
    s = s.lstrip(" \f\v")
    k, sign = 0, 1
    if s[:1] in "+-" and s[:1]:
        sign = -1 if s[0] == "-" else 1
        k = 1
    j = k
    while j < len(s) and s[j].isdigit():
        j += 1
    v = sign * int(s[k:j]) if j > k else 0
    return _i32(v) if -(1 << 63) <= v < (1 << 63) else (-1 if v > 0 else 0)


def _fields(line):
    return [t for t in line.replace("\r", "\t").replace("\n", "\t").split("\t") if t]


def model(records, paf_text, trim=False):
    """records: [(name, seq bytes)] as kseq reads them -> (stdout bytes, report, missing, wpaf, summary lines); the PAF must be well formed"""
    ctgs, tgts = {}, {}
    lines = paf_text.split("\n")           # getline() lines (a '\r' is a field separator, not a line end)
    if lines[-1] == "":
        lines.pop()
    for ln in lines:
        f = _fields(ln)
        rid, tid = f[0], f[5]
        c = ctgs.setdefault(rid, {"p": 0, "n": 0, "tally": {}, "name": None})
        if tid not in tgts:
            tgts[tid] = len(tgts)
        length = _i32(_atoi(f[8]) - _atoi(f[7]))
        if f[4] == "+":
            c["p"] += length
        else:
            c["n"] += length
        c["tally"][tgts[tid]] = c["tally"].get(tgts[tid], 0) + 1
    tnames = sorted(tgts, key=tgts.get)
    clean = []
    for t in tnames:
        if trim:
            t = t.split("_PATERNAL")[0]
            t = t.split("_MATERNAL")[0]
        clean.append(t)
    counter = [0] * len(tnames)
    out, report, missing = [], [], []
    total = neg = miss = 0
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for name, seq in records:
        c = ctgs.get(name)
        if c is None:
            missing.append(name + "\n")
            miss += 1
            continue
        rc = c["p"] < c["n"]
        best = max(c["tally"].items(), key=lambda kv: (kv[1], kv[0]))[0]
        k = counter[best]
        counter[best] += 1
        c["name"] = "%s_%d" % (clean[best], k)
        if rc:
            seq = seq[::-1].translate(comp)
            neg += 1
        report.append("%s\t%s\t%s\t%s\n" % (name, clean[best], "-" if rc else "+", c["name"]))
        out.append(b">" + c["name"].encode() + b"\n" + seq + b"\n")
        total += 1
    wpaf = []
    for ln in lines:
        f = _fields(ln)
        c = ctgs[f[0]]
        qlen, qs, qe = _atoi(f[1]), _atoi(f[2]), _atoi(f[3])
        d = 0 if f[4] == "+" else 1
        if c["p"] < c["n"]:
            d, qs, qe = 1 - d, _i32(qlen - qe), _i32(qlen - qs)
        tp = "P"
        for t in f[12:]:
            if t == "tp:A:P":
                tp = "P"
            elif t == "tp:A:S":
                tp = "S"
        wpaf.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:%s\n" % (
            c["name"] if c["name"] is not None else "(null)", qlen, qs, qe, "+-"[d], f[5], _atoi(f[6]), _atoi(f[7]), _atoi(f[8]), _atoi(f[9]),
            _atoi(f[10]), _atoi(f[11]) & 0xFF, tp))
    return b"".join(out), "".join(report), "".join(missing), "".join(wpaf), ["total: %d" % total, "negative: %d" % neg, "missing: %d" % miss]


# ---- random cases ---------------------------------------------------------------------------------------------------------------------------
LETTERS = b"ACGTACGTACGTacgtNnRYKMSWBDHVU-"


def random_case(seed, d, big=False, fastq=False):
    """write one random case into d -> (argv, inputs, records, paf_text, trim)"""
    rng = random.Random(seed)
    pool = ["c%d" % i for i in range(rng.randint(1, 14))]
    records = []
    for _ in range(rng.randint(1, 16)):
        n = rng.choice([0, 1, 2, 15, 16, 17, 31, 63, 64, 65]) if rng.random() < 0.3 else rng.randint(0, 20000 if big else 700)
        seq = bytes(rng.choice(LETTERS) for _ in range(n))
        records.append((rng.choice(pool), seq))
    tg = ["chr1_PATERNAL", "chr1_MATERNAL", "chr2", "chrX_MATERNAL_PATERNAL", "chrY"][:rng.randint(1, 5)]
    named = [c for c in pool if rng.random() < 0.8] + ["only%d" % i for i in range(rng.randint(0, 3))]
    paf = []
    for c in named:
        for _ in range(rng.randint(1, 5)):
            ts = rng.randint(0, 50)
            te = ts + rng.choice([0, 10, 20, 30, rng.randint(0, 100)])
            sep = "\t\t" if rng.random() < 0.1 else "\t"
            f = [c, str(rng.randint(0, 30000)), str(rng.randint(0, 100)), str(rng.randint(0, 30000)), rng.choice("++--*"), rng.choice(tg),
                 str(rng.randint(1, 10 ** 6)), str(ts), str(te), str(rng.randint(0, 100)), str(rng.randint(0, 100)), str(rng.randint(0, 400))]
            f += rng.sample(["tp:A:P", "tp:A:S", "tp:A:I", "NM:i:3", "cg:Z:10M"], rng.randint(0, 2))
            paf.append(sep.join(f) + ("\r\n" if rng.random() < 0.1 else "\n"))
    rng.shuffle(paf)
    paf_text = "".join(paf)
    width = rng.choice([0, 0, 1, 7, 60, 80])
    parts = []
    for name, seq in records:
        if fastq:
            parts.append(b"@" + name.encode() + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
            continue
        parts.append(b">" + name.encode() + (b" comment" if rng.random() < 0.2 else b"") + b"\n")
        if width and seq:
            parts += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
        else:
            parts.append(seq + b"\n")
    text = b"".join(parts)
    gz = rng.random() < 0.3
    fa = os.path.join(d, "in.fa" + (".gz" if gz else ""))
    with (gzip.open(fa, "wb") if gz else open(fa, "wb")) as fh:
        fh.write(text)
    pf = os.path.join(d, "in.paf")
    with open(pf, "w", newline="") as fh:
        fh.write(paf_text)
    trim = rng.random() < 0.5
    argv = ["fixasm"] + (["--trim-pat-mat"] if trim else []) + ["-r", "{R}", "-m", "{M}", "-w", "{W}", fa, pf]
    return argv, {}, records, paf_text, trim


def check_random(cli, seed, d, env=None, big=False, fastq=False):
    argv, inputs, records, paf_text, trim = random_case(seed, d, big, fastq)
    got = run_case(cli, argv, inputs, d, env)
    out, report, missing, wpaf, summ = model(records, paf_text, trim)
    exp = {"rc": 0, "out": out, "summary": summ, "report": report, "missing": missing, "wpaf": wpaf}
    same(got, exp)
    if os.path.exists(REF_CLI):
        same(run_case(REF_CLI, argv, inputs, d), exp)
