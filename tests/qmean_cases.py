"""`seq -q` test material (CPU): the weight table of include/cornetto_accel.h worked out with `decimal`, the rule in plain Python integers, the
expectation for FASTQ texts (the oracle's kseq restatement, filtered) and for BAM records (bamfq_cases' text of a record, filtered), and the
texts and records of tests/test_gpu_qmean.py and tests/test_qmean_host.py.  Nothing here looks at what the code under test returns."""
import random
import struct
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np

import bam_cases
import bamfq_cases as bq
import oracle_bind as ob
from helpers import fmt_seq

ONE = 10 ** 9
CHUNK = 1024           # QM_CHUNK: bytes of the window per wave of qmean_sum
GROUP = 4096           # bytes of the window per workgroup


def weights():
    """E[q] = round(10^9 * 10^(-q/10)), q = 0 .. 93, at 60 digits (no entry is a tie: checked)"""
    getcontext().prec = 60
    out = []
    for q in range(94):
        x = Decimal(ONE) * Decimal(10) ** (Decimal(-q) / 10)
        assert abs(x - x.to_integral_value(rounding=ROUND_HALF_EVEN)) < Decimal("0.4999999999") or x == x.to_integral_value()
        out.append(int(x.to_integral_value(rounding=ROUND_HALF_EVEN)))
    return out


E = weights()
KNOWN = {0: 1000000000, 1: 794328235, 10: 100000000, 20: 10000000, 30: 1000000, 93: 1}
_CHAR = np.array([E[min(max(c - 33, 0), 93)] for c in range(256)], dtype=np.uint64)


def max_err(t):
    """P of `seq -q t`"""
    import math
    return int(math.floor(1e9 * math.pow(10.0, -t / 10.0) + 0.5))


def qsum(qual):
    """S of a printed quality line: a Python integer (16 * 10^9 * 2^31 fits uint64: the numpy sum is exact)"""
    return int(_CHAR[np.frombuffer(qual, dtype=np.uint8)].sum()) if qual else 0


def passes(s, n_bases, p):
    return p < 0 or s <= p * n_bases


class Want:
    """text; stats = the four counts of the two summary lines; qstats = [reads, bases printed]; keep = the record table's column; sums = the
    records' S (0: dropped before the sum)"""

    def __init__(self):
        self.text, self.stats, self.qstats, self.keep, self.sums = b"", [0, 0, 0, 0], [0, 0], [], []


_FQ = {}


def expect_fastq(text, min_len, p):
    """what `seq -m min_len -q ..` makes of a FASTQ text; p: P, or -1 for no -q"""
    key = (text, min_len, p)
    if key in _FQ:
        return _FQ[key]
    w, out = Want(), []
    for rec in ob.fastx_parse(text)[0]:
        n = len(rec[2])
        w.stats[0] += 1
        w.stats[1] += n
        s, printed = 0, False
        if n >= min_len:
            w.stats[2] += 1
            w.stats[3] += n
            s = qsum(rec[3] or b"")
            printed = not rec[3] or passes(s, n, p)
        if printed:
            out.append(rec)
            w.qstats[0] += 1
            w.qstats[1] += n
        w.keep.append(int(printed))
        w.sums.append(s)
    w.text = fmt_seq(out, 0)
    _FQ[key] = w
    return w


def expect_bam(data, min_len, duplex, p):
    """the same for the inflated bytes of a valid BAM; keep is the `kept` column (-1: passed over)"""
    w, out = Want(), []
    for off, n in bam_cases.record_sizes(data):
        d = data[off + 4:off + n]
        _ref, _pos, l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", d, 0)
        if flag & 0x900:
            w.keep.append(-1)
            w.sums.append(0)
            continue
        w.stats[0] += 1
        w.stats[1] += l_seq
        s, printed = 0, False
        if l_seq >= min_len and (not duplex or bq.find_dx(d, 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq) == 1):
            w.stats[2] += 1
            w.stats[3] += l_seq
            t = bq.fastq_of(d)
            s = qsum(t[len(t) - 1 - l_seq:len(t) - 1])          # the characters `seq --bam` prints
            printed = passes(s, l_seq, p)
            if printed:
                out.append(t)
                w.qstats[0] += 1
                w.qstats[1] += l_seq
        w.keep.append(int(printed))
        w.sums.append(s)
    w.text = b"".join(out)
    return w


def summary(w, min_len, t=None):
    """the stderr lines of `seq`; t: the argument of -q"""
    s = "total reads: %d\t%d bases\t%.2f Gbases\nreads >= %d: %d\t%d bases\t%.2f Gbases\n" % (w.stats[0], w.stats[1], w.stats[1] / 1e9, min_len, w.stats[2], w.stats[3], w.stats[3] / 1e9)
    if t is not None:
        s += "mean qscore >= %g: %d\t%d bases\t%.2f Gbases\n" % (t, w.qstats[0], w.qstats[1], w.qstats[1] / 1e9)
    return s.encode()


def summary_of(err):
    return b"".join(ln + b"\n" for ln in err.split(b"\n") if ln.startswith((b"total reads:", b"reads >= ", b"mean qscore >= ")))


# ---- FASTQ texts ------------------------------------------------------------------------------------------------------------------------------
PRINTABLE = bytes(range(33, 127))


def _rand(rng, alphabet, n):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n)) if n else b""


def _qual(rng, n):
    """n quality characters: of a read that passes Q10 with certainty (Q10 .. Q40), or of one that most likely does not (Q2 .. Q40)"""
    return _rand(rng, b"+.5?I" if rng.integers(0, 2) else b"#%(+.5?I", n)


def rec(name, seq, qual, eol=b"\n"):
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


def placed(at, name, seq, qual, where):
    """a record for offset `at` of a text whose name is padded so that its quality line begins at the next offset that is `where` modulo
    `CHUNK`-like unit: where = (unit, residue)"""
    unit, res = where
    q0 = at + 1 + len(name) + 1 + len(seq) + 3
    pad = (res - q0) % unit
    r = rec(name + b"p" * pad, seq, qual)
    assert (at + len(r) - 1 - len(qual)) % unit == res
    return r


def lane_seam_text():
    """the quality line begins at every offset 0 .. 15 modulo 16 with every length 1 .. 48; about half the reads are below Q10"""
    rng = np.random.default_rng(21)
    out, at = [], 0
    for off in range(16):
        for n in range(1, 49):
            out.append(placed(at, b"l%d_%d" % (off, n), _rand(rng, b"ACGT", n), _qual(rng, n), (16, off)))
            at += len(out[-1])
    return b"".join(out)


def chunk_seam_text():
    """quality lines that straddle a 1 KiB and a 4 KiB multiple of the window by every split of 1 .. 40 bytes in front of it, one that ends and
    one that begins exactly there, and lines that span three and nine chunks"""
    rng = np.random.default_rng(22)
    out, at = [], 0
    for unit in (CHUNK, GROUP):
        for front in list(range(0, 41)) + [57]:
            n = 57
            out.append(placed(at, b"c%d_%d" % (unit, front), _rand(rng, b"ACGT", n), _qual(rng, n), (unit, (unit - front) % unit)))
            at += len(out[-1])
    for n in (2 * CHUNK + 2, 8 * CHUNK + 100, 3 * CHUNK):
        out.append(placed(at, b"span%d" % n, _rand(rng, b"ACGT", n), _qual(rng, n), (CHUNK, CHUNK - 1 if n != 3 * CHUNK else 0)))
        at += len(out[-1])
    return b"".join(out)


def dense_text():
    """300 one-base records of 9 bytes: more than 100 quality lines inside one 1 KiB chunk; every third is Q0"""
    return b"".join(rec(b"d", b"ACGT"[i & 3:(i & 3) + 1], b"!" if i % 3 == 0 else b"I") for i in range(300))


def odd_text(crlf=False, last_newline=True):
    """length-0 records, the quality bytes 0x01, TAB, ' ', 0x7F and 0xFF (clamped to Q0 and Q93), CR LF line ends, a last record without its
    newline"""
    eol = b"\r\n" if crlf else b"\n"
    recs = [rec(b"e0", b"", b"", eol), rec(b"low", b"ACGTA", b"\x01\t  \x01", eol), rec(b"high", b"ACGTA", b"\x7f\xff\x7f\xff~", eol), rec(b"e1", b"", b"", eol),
            rec(b"mix", b"ACGTACGT", b"\x01\xff\t\x7f I!~", eol), rec(b"q10", b"ACGTAC", b"++++++", eol), rec(b"q9", b"ACGTAC", b"+++++*", eol), rec(b"e2", b"", b"", eol),
            rec(b"last", b"ACGTACGTACGTACGTACG", b"5" * 19, eol)]
    if crlf:          # (kseq keeps the CR of a line that holds nothing else: no empty reads here)
        recs = [r for r in recs if not r.startswith(b"@e")]
    text = b"".join(recs)
    return text if last_newline else text[:-len(eol)]


def boundary_text():
    """all-Q10 records of many lengths (equality at P = 10^8), one Q0 among Q40s, a record of 70 000 '!' (sum 7 * 10^13)"""
    out = [rec(b"q10_%d" % n, b"A" * n, b"+" * n) for n in (1, 2, 15, 16, 17, 63, 64, 65, 1000, 4097)]
    out += [rec(b"q0_in_q40_%d" % n, b"C" * n, b"I" * (n // 2) + b"!" + b"I" * (n - n // 2 - 1)) for n in (1, 2, 9, 10, 11, 100, 1000, 10001)]
    out.append(rec(b"all_q0", b"G" * 70000, b"!" * 70000))
    out.append(rec(b"tail", b"ACGT", b"IIII"))
    return b"".join(out)


def random_text():
    """2 000 records of 0 .. 5 000 bases, a quality range of its own per record"""
    rng = np.random.default_rng(23)
    out = []
    for i in range(2000):
        n = int(rng.integers(0, 5001))
        lo = int(rng.integers(33, 60))
        hi = int(rng.integers(lo + 1, 127))
        out.append(b"@r%d c\n" % i + rng.integers(65, 69, n, dtype=np.uint8).tobytes() + b"\n+\n" + rng.integers(lo, hi, n, dtype=np.uint8).tobytes() + b"\n")
    return b"".join(out)


def window_text():
    """120 records of 20 .. 400 bases: a window of 1 000 bytes holds a few, and whole windows are dropped"""
    rng = np.random.default_rng(24)
    out = []
    for i in range(120):
        n = int(rng.integers(20, 401))
        out.append(rec(b"w%d" % i, _rand(rng, b"ACGT", n), _rand(rng, b"!#%", n) if 40 <= i < 60 else _qual(rng, n)))
    return b"".join(out)


def wrapped_text():
    """a record with its bases on two lines in the middle: the device's part ends in front of it -> (text, its offset)"""
    rng = np.random.default_rng(25)
    good = [rec(b"g%d" % i, _rand(rng, b"ACGT", 30 + i), _qual(rng, 30 + i)) for i in range(12)]
    bad = b"@wrapped\nACGTACGT\nACGT\n+\n" + b"!" * 12 + b"\n"
    return b"".join(good[:6]) + bad + b"".join(good[6:]), sum(len(g) for g in good[:6])


def longest_record(text):
    lines = text.split(b"\n")
    return max([sum(len(x) + 1 for x in lines[i:i + 4]) for i in range(0, len(lines), 4)] + [1])


def fastq_ranges(text):
    """[(offset of the quality line, its length)] of a plain text: the ranges of qmean_sum"""
    out, at = [], 0
    lines = text.split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        n = len(lines[i + 1]) - lines[i + 1].endswith(b"\r") * (len(lines[i + 1]) > 1)
        out.append((at + len(lines[i]) + 1 + len(lines[i + 1]) + 1 + len(lines[i + 2]) + 1, n))
        at += sum(len(x) + 1 for x in lines[i:i + 4])
    return out


# ---- BAM records ------------------------------------------------------------------------------------------------------------------------------
def bam_record(name, bases, quals, flag=4, aux=b"", cigar=()):
    """bamfq_cases.record() with its CIGAR operations written out (they shift the quality array)"""
    l_seq = len(bases)
    quals = bytes([0xFF]) * l_seq if quals is None else bytes(quals)
    nm = name + b"\0"
    data = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, len(cigar), flag, l_seq, -1, -1, 0)
    data += nm + b"".join(struct.pack("<I", c) for c in cigar) + bq.pack_bases(bases) + quals + aux
    return struct.pack("<i", len(data)) + data


def bam_records():
    """reverse-strand records, absent qualities, raw qualities 94 .. 254, odd l_seq, long names and CIGARs, auxiliary fields of low quality
    bytes behind the qualities, SECONDARY records, dx fields"""
    rng = random.Random(26)
    one, zero = bq.aux_int(b"dx", "c", 1), bq.aux_int(b"dx", "c", 0)
    junk = b"zzZ" + bytes([1]) * 40 + b"\0"          # (bytes that would be Q1 if they were counted)
    out = []
    for k in range(60):
        n = (0, 1, 2, 15, 16, 17, 31, 33, 47, 48, 49, 257, 1023, 1025, 3001)[k % 15]
        lo = rng.choice((0, 3, 8, 12, 30))
        q = bytes(rng.randrange(lo, lo + 12) for _ in range(n))
        out.append(bam_record(b"n" * (1 + 17 * (k % 14)) + b"%d" % k, "".join(rng.choice("ACGT") for _ in range(n)), q, flag=(4, 0x14)[k & 1],
                              aux=(one, zero, b"", junk + one)[k % 4], cigar=[(n << 4) | 4] * (k % 5)))
    out.append(bam_record(b"absent", "ACGTN" * 7, None))
    out.append(bam_record(b"absent_rev", "ACGTN" * 201, None, flag=0x14, aux=one))
    out.append(bam_record(b"high", "ACGT" * 41, bytes(range(94, 255)) + bytes([93, 94, 254])))
    out.append(bam_record(b"high_rev", "ACGT" * 41, bytes(range(94, 255)) + bytes([0, 0, 0]), flag=0x14, aux=one))
    out.append(bam_record(b"ff_later", "C" * 18, bytes([7, 0xFF] + [9] * 16)))
    out.append(bam_record(b"secondary", "ACGT" * 10, bytes([0] * 40), flag=0x104, aux=one))
    out.append(bam_record(b"supplementary", "ACGT" * 10, bytes([40] * 40), flag=0x804))
    out.append(bam_record(b"q10", "A" * 100, bytes([10] * 100), aux=one))
    out.append(bam_record(b"q0_in_q40", "A" * 100, bytes([40] * 99 + [0]), flag=0x14))
    out.append(bam_record(b"long", "ACGT" * 9000, bytes(rng.randrange(5, 30) for _ in range(36000)), flag=0x14, aux=junk))
    return out


def bam_ranges(data):
    """[(offset of the quality array, l_seq)] of the records of the inflated BAM `data` that have qualities"""
    out = []
    for off, n in bam_cases.record_sizes(data):
        d = data[off + 4:off + n]
        l_read_name, n_cigar, l_seq = d[8], struct.unpack_from("<H", d, 12)[0], struct.unpack_from("<I", d, 16)[0]
        q = off + 4 + 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2
        out.append((q, 0 if l_seq and data[q] == 0xFF else l_seq))
    return out
