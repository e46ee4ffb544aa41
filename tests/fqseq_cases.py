"""FASTQ texts for `seq --fastq` / cornetto_fqseq_* (tests/test_gpu_fqseq.py, tests/test_fqseq_host.py) and what `seq -m` prints for them:
the records of the oracle's kseq restatement (oracle_bind.fastx_parse), formatted as src/seq.c:120-129 prints them (helpers.fmt_seq)."""
import os

import numpy as np

import oracle_bind as ob
from helpers import fmt_seq, tricky_fastx

TILE = 16384           # CORNETTO_FQSEQ_TILE: output bytes per workgroup of fqseq_text (tests/test_gpu_fqseq.py checks it against the library)
SCAN_TILE = 4096       # cnscan::SC_TILE: counters per tile of the device scan
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_EXP = {}


def expected(text, min_len):
    """(stdout of `seq -m min_len`, [reads, bases, reads kept, bases kept], number of records) by the oracle"""
    key = (text, min_len)
    if key not in _EXP:
        recs, _ = ob.fastx_parse(text)
        kept = [len(s) for _, _, s, _ in recs if len(s) >= min_len]
        _EXP[key] = (fmt_seq(recs, min_len), [len(recs), sum(len(s) for _, _, s, _ in recs), len(kept), sum(kept)], len(recs))
    return _EXP[key]


def record(name, comment, seq, qual, sep=b" ", eol=b"\n", plus=b""):
    return b"@" + name + (sep + comment if comment is not None else b"") + eol + seq + eol + b"+" + plus + eol + qual + eol


def longest_record(text):
    """bytes of the longest group of four lines (what the smallest window must hold)"""
    lines = text.split(b"\n")
    sizes = [sum(len(x) + 1 for x in lines[i:i + 4]) for i in range(0, len(lines), 4)]
    return max(sizes + [1])


def _rand(rng, alphabet, n):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


QUAL = bytes(range(33, 74))


# ---- 1. the golden reads and the strict random texts -------------------------------------------------------------------------------------------
def golden_reads():
    return open(os.path.join(GOLDEN, "reads.fq"), "rb").read()


def strict_texts():
    """the seeds and sizes of test_gpu_fastq.py::test_strict_text_is_indexed_completely"""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(40):
        text = tricky_fastx(rng, int(rng.integers(1, 60)), strict=True)
        if not text.endswith(b"\n") and text.endswith(b"+"):
            text += b"\n"
        out.append(text)
    return out


# ---- 2. header and line rules ---------------------------------------------------------------------------------------------------------------------
RULES = {
    "no_comment": b"@r1\nACGT\n+\nIIII\n",
    "space": b"@r2 comment here\nACGTA\n+\nIIIII\n",
    "tab": b"@r3\tcomment\twith tabs\nACGTAC\n+\nIIIIII\n",
    "two_spaces": b"@r4  two\nAC\n+\nII\n",                       # the comment begins with a space
    "empty_comment": b"@r5 \nACG\n+\nIII\n",                     # no tab printed
    "crlf": b"@r6 c d\r\nACGTACG\r\n+\r\nIIIIIII\r\n",
    "comment_cr": b"@r7 \r\nACGT\n+\nIIII\n",                    # a comment that is exactly "\r"
    "plus_name": b"@r8 x\nACGTACGT\n+r8 x\nIIIIIIII\n",
    "empty_read": b"@r\n\n+\n\n",
    "no_last_newline": b"@r9 last\nACGTA\n+\nIIIII",
}
RULES_MIXED = b"".join(RULES[k] for k in RULES)          # (the record without its last newline stands last)
RULE_MIN_LENS = (0, 4)


# ---- 3. tile seams ----------------------------------------------------------------------------------------------------------------------------------
SEAM_PARTS = ("at", "name", "tab", "comment", "nl1", "base_first", "base_last", "nl2", "plus", "nl3", "qual_first", "qual_last", "nl4")


def _part_offset(part, nl, cl, ln):
    """offset of the part in the text of a record with a comment"""
    nl1 = 1 + nl + 1 + cl
    nl2 = nl1 + ln + 1
    nl3 = nl2 + 2
    return {"at": 0, "name": 2, "tab": 1 + nl, "comment": 1 + nl + 2, "nl1": nl1, "base_first": nl1 + 1, "base_last": nl1 + ln, "nl2": nl2, "plus": nl2 + 1,
            "nl3": nl3, "qual_first": nl3 + 1, "qual_last": nl3 + ln, "nl4": nl3 + ln + 1}[part]


def seam_text(part, tile=TILE):
    """about three tiles of records of 40-300 bytes, every one kept at -m 0; the comment of the first is padded (as seam_text of
    test_gpu_fastq.py pads its headers) so that output byte `tile` is the named part of a record"""
    rng = np.random.default_rng(SEAM_PARTS.index(part) + 100)
    recs = []
    size = 0
    while size < 3 * tile:
        ln = int(rng.integers(8, 130))
        name, com = b"s%d" % len(recs) + b"n" * int(rng.integers(1, 9)), b"c" * int(rng.integers(4, 20))
        recs.append([name, com, _rand(rng, b"ACGT", ln), _rand(rng, QUAL, ln)])
        size += 1 + len(name) + 1 + len(com) + 1 + ln + 3 + ln + 1
    out_size = lambda r: 1 + len(r[0]) + 1 + len(r[1]) + 1 + len(r[2]) + 3 + len(r[3]) + 1
    pre, k = 0, 0
    while pre + out_size(recs[k]) <= tile - 700:
        pre += out_size(recs[k])
        k += 1
    pre += out_size(recs[k])
    k += 1                                                      # tile - 700 < pre <= tile - 700 + 300: record k begins at most 700 bytes in front of the seam
    pad = tile - pre - _part_offset(part, len(recs[k][0]), len(recs[k][1]), len(recs[k][2]))
    assert pad > 0
    recs[0][1] += b"x" * pad
    text = b"".join(record(*r) for r in recs)
    out = expected(text, 0)[0]
    start = pre + pad
    assert out[start:start + 1] == b"@" and start + _part_offset(part, len(recs[k][0]), len(recs[k][1]), len(recs[k][2])) == tile
    return text


def long_read_text(tile=TILE):
    """one read of 2.5 tiles of bases between short ones: whole tiles lie inside the bases and inside the qualities"""
    rng = np.random.default_rng(7)
    n = tile * 5 // 2
    small = [record(b"s%d" % i, b"c", _rand(rng, b"ACGT", 30 + i), _rand(rng, QUAL, 30 + i)) for i in range(6)]
    return b"".join(small[:3]) + record(b"long", b"read of 2.5 tiles", _rand(rng, b"ACGTN", n), _rand(rng, QUAL, n)) + b"".join(small[3:])


def tiny_text():
    """10 000 tiny records, more than one tile of the device scan; -m 2 drops every second one"""
    return b"".join(record(b"t%d" % i, None, b"AC"[:1 + (i & 1)], b"IJ"[:1 + (i & 1)]) for i in range(10000))


# ---- 4. source alignment ----------------------------------------------------------------------------------------------------------------------------
ALIGN_MIN_LEN = 40


def align_text():
    """64 records with name lengths 1..16 and a dropped record between kept ones: every residue of (source - destination) mod 16 occurs in
    the bases and in the qualities (asserted)"""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(64):
        name = b"abcdefghijklmnop"[:1 + i % 16]
        if i % 3 == 1:          # dropped, and 1 mod 16 bytes long: the kept record behind it is read one residue further on
            recs.append(record(name, b"k" * (16 - len(name) % 16), b"ACGTA", b"IIIII"))
            assert len(recs[-1]) % 16 == 1
            continue
        ln = int(rng.integers(48, 90))
        recs.append(record(name, b"k" * (i % 5) if i % 5 else None, _rand(rng, b"ACGT", ln), _rand(rng, QUAL, ln)))
    text = b"".join(recs)
    src, dst, res = 0, 0, [set(), set()]
    parsed, _ = ob.fastx_parse(text)
    for raw, (name, com, seq, qual) in zip(recs, parsed):
        if len(seq) >= ALIGN_MIN_LEN:
            s_seq, s_qual = src + raw.index(b"\n") + 1, src + len(raw) - 1 - len(qual)
            d_seq = dst + 1 + len(name) + (1 + len(com) if com else 0) + 1
            res[0].add((s_seq - d_seq) % 16)
            res[1].add((s_qual - (d_seq + len(seq) + 3)) % 16)
            dst = d_seq + 2 * len(seq) + 4
        src += len(raw)
    assert res[0] == set(range(16)) and res[1] == set(range(16)), res
    return text


# ---- 6. BGZF input ----------------------------------------------------------------------------------------------------------------------------------
def block_size(text):
    return 1000 if len(text) < 3 * TILE + 4000 else 60000


def bgzf_seam_case():
    """block borders inside a name, on a newline, inside the bases and inside the qualities -> (text, block sizes)"""
    recs = [record(b"name_of_%d" % i, b"c%d" % i, b"ACGTTGCA" * 6, b"IJKLMNOP" * 6) for i in range(8)]
    text = b"".join(recs)
    n = len(recs[0])
    cuts = [4, n + recs[1].index(b"\n"), 2 * n + recs[2].index(b"\n") + 20, 3 * n + len(recs[3]) - 30, 5 * n]
    assert text[cuts[1]:cuts[1] + 1] == b"\n"
    return text, [b - a for a, b in zip([0] + cuts, cuts)]


# ---- 8. not plain -------------------------------------------------------------------------------------------------------------------------------------
def irregular_texts():
    """the population of test_gpu_fastq.py::test_irregular_text_stops_at_the_first_irregular_record"""
    rng = np.random.default_rng(12)
    return [tricky_fastx(rng, int(rng.integers(0, 25)), strict=False) for _ in range(120)]


def zero_byte_texts():
    """a byte 0 in the name, in the bases and in the qualities of the third record -> [(text, offset of the third record)]"""
    good = [record(b"z%d" % i, b"c", b"ACGTACGTAC", b"IIIIIIIIII") for i in range(5)]
    out = []
    for bad in (record(b"z\x002", b"c", b"ACGTACGTAC", b"IIIIIIIIII"), record(b"z2", b"c", b"ACGT\x00CGTAC", b"IIIIIIIIII"), record(b"z2", b"c", b"ACGTACGTAC", b"IIIIIII\x00II")):
        out.append((good[0] + good[1] + bad + good[3] + good[4], len(good[0]) + len(good[1])))
    return out


# ---- 9. a damaged block ---------------------------------------------------------------------------------------------------------------------------------
def four_block_text():
    rng = np.random.default_rng(9)
    text = b"".join(record(b"d%d" % i, b"c", _rand(rng, b"ACGT", 40 + i % 7), _rand(rng, QUAL, 40 + i % 7)) for i in range(40))
    size = len(text) // 4 + 1
    return text, [size] * 4


def whole_records_in(text, n):
    """the text of the records that lie wholly inside text[:n]"""
    end = 0
    lines = text[:n].split(b"\n")[:-1]
    for i in range(0, len(lines) - len(lines) % 4, 4):
        end += sum(len(x) + 1 for x in lines[i:i + 4])
    return text[:end]


def all_cases():
    """name -> (text, min_lens): every case of sections 1-4"""
    cases = {"golden": (golden_reads(), (0, 100, 30000))}
    for i, t in enumerate(strict_texts()):
        cases["strict%02d" % i] = (t, (0, 60))
    for k, t in RULES.items():
        cases["rule_" + k] = (t, RULE_MIN_LENS)
    cases["rules_mixed"] = (RULES_MIXED, RULE_MIN_LENS)
    for p in SEAM_PARTS:
        cases["seam_" + p] = (seam_text(p), (0,))
    cases["long_read"] = (long_read_text(), (0, 1000))
    cases["tiny"] = (tiny_text(), (2,))
    cases["align"] = (align_text(), (ALIGN_MIN_LEN,))
    return cases
