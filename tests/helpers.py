"""Shared test helpers: record readers with the reference reader's framing rules and text formatters that
mirror the reference's printf formats, so oracle / GPU outputs can be diffed against golden stdout."""
import gzip
import os

import numpy as np


def _open(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def read_fastx(path):
    """[(name, comment, seq, qual)] with klib kseq framing (src/kseq.h:184-224, :93-141): jump to the next
    '>'/'@', name up to the first isspace() byte, comment = rest of that line, sequence lines until a line
    that starts with '>', '@' or '+', a trailing CR dropped from each line once more than one byte is held,
    '+' line skipped, quality read by length; a truncated quality string ends the stream."""
    with _open(path) as f:
        d = f.read()
    n = len(d)
    recs = []
    pos = 0
    SPACE = b" \t\n\v\f\r"

    def getline(p, acc):
        """append bytes up to the next LF to acc (kseq ks_getuntil2 KS_SEP_LINE, append=1)"""
        e = d.find(b"\n", p)
        if e < 0:
            e = n
        acc += d[p:e]
        if len(acc) > 1 and acc[-1:] == b"\r":
            del acc[-1]
        return min(e + 1, n + 1)

    last = 0
    while True:
        if last == 0:
            while pos < n and d[pos] not in b">@":
                pos += 1
            if pos >= n:
                break
            pos += 1
        if pos >= n:
            break
        e = pos
        while e < n and d[e] not in SPACE:
            e += 1
        name = d[pos:e]
        delim = d[e] if e < n else 0
        pos = min(e + 1, n)
        comment = bytearray()
        if delim != 0x0A and e < n:
            pos = getline(pos, comment)
        seq = bytearray()
        c = -1
        while pos < n:
            c = d[pos]
            pos += 1
            if c in b">+@":
                break
            if c == 0x0A:
                c = -1
                continue
            seq.append(c)
            pos = getline(pos, seq)
            c = -1
        last = c if c in (0x3E, 0x40) else 0
        if c != 0x2B:
            recs.append((name, bytes(comment), bytes(seq), None))
            if pos >= n and last == 0:
                break
            continue
        e = d.find(b"\n", pos)
        if e < 0:
            break
        pos = e + 1
        qual = bytearray()
        while pos <= n and len(qual) < len(seq):
            if pos >= n:
                break
            pos = getline(pos, qual)
        last = 0
        if len(qual) != len(seq):
            break
        recs.append((name, bytes(comment), bytes(seq), bytes(qual)))
    return recs


def read_bedgraph_pair(tot_path, mq_path):
    """-> [(name, depth_u16, mq_u16)] with the reference reader's 65535 clamp (src/boringbits_main.c:261-268)"""
    def load(p):
        with _open(p) as f:
            names, vals = [], []
            for ln in f:
                a = ln.split()
                names.append(a[0])
                vals.append(int(a[3]))
        return names, np.minimum(np.array(vals, dtype=np.int64), 65535).astype(np.uint16)
    n1, d = load(tot_path)
    n2, q = load(mq_path)
    assert n1 == n2
    out = []
    start = 0
    for i in range(1, len(n1) + 1):
        if i == len(n1) or n1[i] != n1[start]:
            out.append((n1[start], d[start:i].copy(), q[start:i].copy()))
            start = i
    return out


def token_at(text, at, nlines=None):
    """the (first nlines) lines of a bedgraph with two spaces between the fields, and as many behind one contig name as it takes for the
    field behind it to start at byte `at` of the text"""
    out, pos, done = [], 0, False
    for ln in text.splitlines()[:nlines]:
        f = ln.split()
        line = b"  ".join(f) + b"\n"
        if not done and pos + len(line) + len(f[0]) + 2 > at:        # the last line whose second field can still be moved there
            line = f[0] + b" " * (at - pos - len(f[0])) + b"  ".join(f[1:]) + b"\n"
            done = True
        out.append(line)
        pos += len(line)
    text = b"".join(out)
    assert done and text[at - 1:at] == b" " and not text[at:at + 1].isspace()
    return text


def fmt_telofind(name, length, hits):
    """src/find_telomere.c:51,56"""
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (name, length, h["strand"], h["start"], h["end"], h["end"] - h["start"])
                    for h in hits)


def fmt_g3(x):
    """C's %.3g"""
    return ("%.3g" % x).encode()


def fmt_telowin(name, length, wins):
    """src/telomere_windows.c:38"""
    return b"".join(b"Window\t%s\t%d\t%d\t%d\t%s\n" % (name, length, w["start"], w["end"],
                                                     fmt_g3(float(w["car"]) / float(w["end"] - w["start"])))
                    for w in wins)


def fmt_sdust(name, res):
    """src/sdust/sdust.c:201 — both halves printed as (int)"""
    out = []
    for r in res:
        r = int(r)
        s = (r >> 32) & 0xFFFFFFFF
        f = r & 0xFFFFFFFF
        s = s - (1 << 32) if s >= 1 << 31 else s
        f = f - (1 << 32) if f >= 1 << 31 else f
        out.append(b"%s\t%d\t%d\n" % (name, s, f))
    return b"".join(out)


def golden(golden_dir, name):
    with open(os.path.join(golden_dir, name), "rb") as f:
        return f.read()


def read_telobreaks_inputs(lens_path, sdust_path, telo_path):
    """the three text inputs of `cornetto telobreaks` as the reference's sscanf calls see them
    (src/telomere_breaks.c:66,82,97): white-space separated leading fields of every line"""
    names, lens = [], []
    for line in open(lens_path, "rb"):
        f = line.split()
        if len(f) >= 2:
            names.append(f[0]); lens.append(int(f[1]))
    sd = [(f[0], int(f[1]), int(f[2])) for f in (l.split() for l in open(sdust_path, "rb")) if len(f) >= 3]
    tel = [(f[0], int(f[3]), int(f[4]), int(f[5])) for f in (l.split() for l in open(telo_path, "rb")) if len(f) >= 6]
    return names, lens, sd, tel


def fmt_telobreaks(name, length, first, last):
    return b"Found telomere positions %d to %d is a telomere in %s of length %d\n" % (first, last, name, length)   # :142


def fmt_seq(recs, min_len):
    """stdout of `cornetto seq -m min_len` for kseq records (name, comment, seq, qual): src/seq.c:120-129"""
    out = []
    for name, com, seq, qual in recs:
        if len(seq) >= min_len:
            out.append(b"@" + name + (b"\t" + com if com else b"") + b"\n" + seq + b"\n+\n" + (qual if qual is not None else b"(null)") + b"\n")
    return b"".join(out)


def fmt_fa2bed(recs):
    """stdout of `cornetto fa2bed`: src/assbed.c:99"""
    return b"".join(b"%s\t0\t%d\n" % (name, len(seq)) for name, com, seq, qual in recs)


def tricky_fastx(rng, n_rec, strict=False, lowc=0.0):
    """FASTA/FASTQ text exercising the framing rules of kseq: CRLF, comments, empty reads, '@' and '>' inside qualities,
    multi-line sequences, blank lines, records without qualities, a last line without newline"""
    alpha = b"ACGTacgtN"
    qalpha = bytes(range(33, 74))
    out = []
    for i in range(n_rec):
        ln = int(rng.choice([0, 1, 2, 5, 60, 61, 200, 1000])) if rng.random() < 0.4 else int(rng.integers(1, 400))
        seq = bytes(alpha[k] for k in rng.integers(0, len(alpha), ln))
        if ln >= 40 and rng.random() < lowc:      # a low-complexity stretch, so that sdust has something to report
            a = int(rng.integers(0, ln - 30))
            b = int(rng.integers(a + 20, ln + 1))
            unit = [b"A", b"TA", b"CAG", b"t"][int(rng.integers(0, 4))]
            seq = seq[:a] + (unit * (b - a))[:b - a] + seq[b:]
        qual = bytes(qalpha[k] for k in rng.integers(0, len(qalpha), ln))
        eol = b"\r\n" if rng.random() < 0.15 else b"\n"
        name = b"r%d" % i
        kind = rng.random()
        if kind < 0.3:
            head = name
        elif kind < 0.6:
            head = name + b" runid=abc ch=%d" % int(rng.integers(1, 512))
        elif kind < 0.7:
            head = name + b"\tcomment with\ttabs "
        elif kind < 0.8:
            head = name + b"  two spaces"
        else:
            head = name + b" "
        if strict or rng.random() < 0.75:
            out.append(b"@" + head + eol + seq + eol + b"+" + (name if rng.random() < 0.2 else b"") + eol + qual + eol)
        else:
            v = int(rng.integers(0, 7))
            if v == 0:      # FASTA record, multi-line
                out.append(b">" + head + eol + b"".join(seq[k:k + 60] + eol for k in range(0, len(seq), 60)))
            elif v == 1:    # multi-line FASTQ
                h = len(seq) // 2
                out.append(b"@" + head + eol + seq[:h] + eol + seq[h:] + eol + b"+" + eol + qual[:h] + eol + qual[h:] + eol)
            elif v == 2:    # blank lines around
                out.append(eol + b"@" + head + eol + seq + eol + eol + b"+" + eol + qual + eol + eol)
            elif v == 3:    # garbage between records
                out.append(b"junk line\n@" + head + eol + seq + eol + b"+" + eol + qual + eol)
            elif v == 4 and ln > 0:    # quality beginning with '@'
                out.append(b"@" + head + eol + seq + eol + b"+" + eol + b"@" + qual[1:] + eol)
            elif v == 5 and ln > 0:    # quality beginning with '>' / '+'
                out.append(b"@" + head + eol + seq + eol + b"+" + eol + (b">" if i & 1 else b"+") + qual[1:] + eol)
            else:
                out.append(b"@" + head + eol + seq + eol + b"+" + eol + qual + eol)
    text = b"".join(out)
    if text.endswith(b"\n") and rng.random() < 0.3:
        text = text[:-1]
    return text


# ---- the random cases of the differential tests against the reference's own code (tests/test_oracle_golden.py).  Where oracle/_ref is
# not built the tests take the cases and the reference's outputs recorded by tests/golden/make_golden_random.py (ref_*_random.npz)
def sdust_random_cases():
    """-> [(sequence uint8, T, W)]: 300 sequences of up to 3000 bases (uniform ACGT, any letter, STR mosaics, two letters)"""
    rng = np.random.default_rng(7)
    alpha = np.frombuffer(b"ACGTacgtNNRY", dtype=np.uint8)
    cases = []
    for it in range(300):
        n = int(rng.integers(0, 3000))
        kind = it % 4
        if kind == 0:
            s = alpha[rng.integers(0, 4, size=n)]
        elif kind == 1:
            s = alpha[rng.integers(0, len(alpha), size=n)]
        elif kind == 2:   # STR mosaic
            parts = []
            while sum(map(len, parts)) < n:
                u = alpha[rng.integers(0, 4, size=int(rng.integers(1, 6)))]
                parts.append(np.tile(u, int(rng.integers(1, 40))))
                if rng.random() < 0.2:
                    parts.append(np.frombuffer(b"N" * int(rng.integers(1, 5)), dtype=np.uint8))
            s = np.concatenate(parts)[:n] if parts else np.zeros(0, np.uint8)
        else:             # two-letter low complexity
            s = alpha[rng.integers(0, 2, size=n)]
        s = np.ascontiguousarray(s, dtype=np.uint8)
        T = int(rng.choice([20, 20, 10, 5, 30]))
        W = int(rng.choice([64, 64, 32, 16, 100, 8]))
        cases.append((s, T, W))
    return cases


def ref_sdust(refso, cases):
    """the reference's sdust() (oracle/_ref/libcornetto_ref.so) on every case -> [uint64 intervals]"""
    import ctypes as C
    ref = C.CDLL(refso)
    ref.sdust.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    ref.sdust.restype = C.POINTER(C.c_uint64)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    out = []
    for s, T, W in cases:
        cnt = C.c_int()
        r = ref.sdust(None, s.tobytes() + b"\0", len(s), T, W, C.byref(cnt))
        out.append(np.array([r[i] for i in range(cnt.value)], dtype=np.uint64))
        libc.free(r)
    return out


def fastx_random_texts():
    """-> [bytes]: 150 FASTA/FASTQ texts of up to 11 records (tricky_fastx; every third one strict FASTQ)"""
    rng = np.random.default_rng(3)
    return [tricky_fastx(rng, int(rng.integers(0, 12)), strict=(it % 3 == 0)) for it in range(150)]


def seq_prints_records(text, recs, rc):
    """`seq` prints stale memory for FASTA records and for a read whose quality the end of the file cuts off"""
    return all(q is not None for _, _, _, q in recs) and not text.endswith(b"+\n") and rc == -1


def pack_bytes(items):
    """[bytes-like or None] -> (uint8 concatenation, int64 offsets[n + 1], bool present[n]) for an .npz fixture"""
    parts = [np.frombuffer(bytes(x), dtype=np.uint8) if x is not None else np.zeros(0, np.uint8) for x in items]
    offs = np.zeros(len(parts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs, np.array([x is not None for x in items], dtype=bool)


def unpack_bytes(data, offs, present=None):
    return [bytes(data[offs[i]:offs[i + 1]]) if present is None or present[i] else None for i in range(len(offs) - 1)]


# ---- the CLI goldens (stdout of the unmodified reference: tests/golden/make_golden.py), shared by the device tests
# (tests/test_gpu_cli.py) and the host-path tests (tests/test_cli_accel_no.py)
FASTA_SIDE = [
    (["telofind", "probe.fa"], "probe.telofind.exp"),
    (["telofind", "mix.fa.gz"], "mix.telofind.exp"),
    (["telofind", "mix.fa.gz", "ttaggg"], "mix.lower_motif.telofind.exp"),
    (["telofind", "mix.fa.gz", "TTAGGGTTAGGG"], "mix.k12.telofind.exp"),
    (["telofind", "mix.fa.gz", "TTAGGG" * 6], "mix.k36.telofind.exp"),
    (["telofind", "mix.fa.gz", "GGGTTA" * 11 + "G"], "mix.k67.telofind.exp"),
    (["telofind", "mix.fa.gz", "AAAA"], "mix.AAAA.telofind.exp"),
    (["telofind", "mix.fa.gz", "GNG"], "mix.GNG.telofind.exp"),
    (["telofind", "probe_selfoverlap.fa", "ACACA"], "probe_selfoverlap.ACACA.telofind.exp"),
    (["sdust", "probe.fa"], "probe.sdust.exp"),
    (["sdust", "probe_sdust.fa"], "probe_sdust.sdust.exp"),
    (["sdust", "-w", "32", "-t", "10", "probe_sdust.fa"], "probe_sdust.w32t10.sdust.exp"),
    (["sdust", "mix.fa.gz"], "mix.sdust.exp"),
    (["sdust", "mix.fa.gz", "-w", "32", "-t", "10"], "mix.w32t10.sdust.exp"),
    (["sdust", "-w", "100", "-t", "25", "mix.fa.gz"], "mix.w100t25.sdust.exp"),
    (["sdust", "reads.fq"], "reads.sdust.exp"),
    (["telowin", "probe.telomere", "99.9", "0.4"], "probe.telowin.exp"),
    (["telowin", "probe.telomere", "100", "0.5"], "probe.i100t05.telowin.exp"),
    (["telowin", "probe.telomere", "95"], "probe.i95.telowin.exp"),
    (["telowin", "mix.telofind.exp", "99.9", "0.4"], "mix.telowin.exp"),
    (["telowin", "mix.telofind.exp", "99.9", "0.1"], "mix.t01.telowin.exp"),
]

def build_asan_cli():
    """`make asan=1` under a file lock: pytest-xdist workers of two test modules would otherwise link the same binary at the same time
    (and one of them would run a half-written file)"""
    import fcntl
    import subprocess
    import cornetto_amd
    d = os.path.dirname(cornetto_amd.CLI_PATH)
    with open(os.path.join(d, ".asan.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", d, "-s", "asan=1"])
    return cornetto_amd.CLI_PATH + "_asan"


def panel_argv(plain, args):
    """"T" / "Q" stand for the uncompressed cov-total.bg / cov-mq20.bg, "T2" / "Q2" for sparse-total.bg / sparse-mq20.bg"""
    names = {"T": "cov-total.bg", "Q": "cov-mq20.bg", "T2": "sparse-total.bg", "Q2": "sparse-mq20.bg"}
    return [plain[names[x]] if x in names else x for x in args]


# command lines on which the reference dies of an assert of get_regs() (src/boringbits_main.c:353): SIGABRT, nothing on stdout
PANEL_ABORT = [
    (["noboringbits", "T", "-q", "Q", "-w", "300", "-i", "350"], "bg.abort_w300i350.exp"),
    (["boringbits", "T", "-q", "Q", "-w", "64", "-i", "1000", "-m", "100"], "bg.abort_w64i1000.exp"),
    (["noboringbits", "T2", "-q", "Q2", "-w", "64", "-i", "999"], "sparse.abort_w64i999.exp"),
]

PANEL = [
    (["boringbits", "T", "-q", "Q", "-m", "10000", "-e", "1000", "-L", "0.6", "-Q", "0.6", "-H", "1.6"], "bg.boring_t1.exp"),
    (["noboringbits", "-H", "2.5", "-L", "0.5", "-Q", "0.5", "T", "-q", "Q", "-m", "10000", "-e", "1000"], "bg.fun_t2.exp"),
    (["noboringbits", "T", "-q", "Q"], "bg.fun_default.exp"),
    (["boringbits", "T", "-q", "Q"], "bg.boring_default.exp"),
    (["noboringbits", "T", "-q", "Q", "-w", "300", "-i", "7", "-L", "0.33", "-H", "1.45", "-Q", "0.9", "-m", "5000", "-e", "500"], "bg.fun_w300i7.exp"),
    (["boringbits", "T", "-q", "Q", "-w", "300", "-i", "7", "-L", "0.33", "-H", "1.45", "-Q", "0.9", "-m", "5000", "-e", "500"], "bg.boring_w300i7.exp"),
    (["noboringbits", "T", "-q", "Q", "-w", "1000", "-i", "1000", "-m", "2000", "-e", "10000"], "bg.fun_w1000i1000.exp"),
    # the options the reference accepts and ignores (src/boringbits_main.c:590-632)
    (["noboringbits", "T", "-q", "Q", "-t", "4", "-K", "10", "-B", "1M", "-o", "/dev/null", "--debug-break", "1", "--profile-cpu", "yes"], "bg.fun_default.exp"),
    # -i larger than -w: sparse windows (:338-369)
    (["noboringbits", "T", "-q", "Q", "-w", "300", "-i", "301", "-m", "5000", "-e", "500"], "bg.fun_w300i301.exp"),
    (["boringbits", "T", "-q", "Q", "-w", "300", "-i", "301", "-m", "5000", "-e", "500", "-L", "0.33", "-H", "1.45"], "bg.boring_w300i301.exp"),
    (["noboringbits", "T2", "-q", "Q2", "-w", "64", "-i", "1000", "-m", "1000", "-e", "200"], "sparse.fun_w64i1000.exp"),
    (["boringbits", "T2", "-q", "Q2", "-w", "64", "-i", "1000", "-m", "1000", "-e", "200", "-L", "0.2", "-H", "3"], "sparse.boring_w64i1000.exp"),
    (["noboringbits", "T2", "-q", "Q2", "-w", "64", "-i", "1000", "-m", "100000"], "sparse.fun_w64i1000_short.exp"),
    # -e beyond every contig, w % inc = 1 (the head sums), a contig of exactly w + 51
    (["noboringbits", "T2", "-q", "Q2", "-w", "1982", "-i", "7", "-e", "5000", "-m", "1000"], "sparse.fun_w1982i7e5000.exp"),
    (["boringbits", "T2", "-q", "Q2", "-w", "1982", "-i", "7", "-e", "5", "-m", "1000", "-L", "0.2", "-H", "3"], "sparse.boring_w1982i7.exp"),
    (["noboringbits", "T2", "-q", "Q2"], "sparse.fun_default.exp"),
]
