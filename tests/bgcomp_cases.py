"""Helpers of the compressed depth file tests (tests/test_bgcomp_host.py, tests/test_gpu_bgcomp.py): the golden depth texts as plain, BGZF
and gzip files, BGZF chains with their block seams at chosen bytes, and the damaged variants of a chain."""
import gzip
import os

import numpy as np

import bgzf_cases as bc

DEPTH_FILES = ("cov-total.bg", "cov-mq20.bg", "sparse-total.bg", "sparse-mq20.bg")
_TEXTS = {}


def golden_text(golden_dir, fn):
    """the depth text of tests/golden/<fn>.gz (ordinary gzip), inflated once"""
    if fn not in _TEXTS:
        _TEXTS[fn] = gzip.open(os.path.join(golden_dir, fn + ".gz")).read()
    return _TEXTS[fn]


def seeded_sizes(n, seed, lo=1, hi=4000):
    """block sizes from lo to hi bytes that cover n bytes"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left > 0:
        k = int(rng.integers(lo, hi + 1))
        out.append(k)
        left -= k
    return out


def sizes_from_cuts(cuts, n):
    """block sizes whose seams fall at the byte offsets `cuts` of a text of n bytes (equal offsets: an empty block between them); bgzf() puts
    what lies behind the last cut into blocks of its own"""
    at, out = 0, []
    for c in sorted(cuts):
        assert at <= c <= n
        out.append(c - at)
        at = c
    return out


def bgzf(text, sizes, eof=True):
    """bgzf_cases.write() that also takes sizes of 0 (an empty member in mid-chain)"""
    out, at = [], 0
    for n in sizes:
        out.append(bc.member(text[at:at + n]))
        at += n
    if at < len(text):
        out.append(bc.write(text[at:], eof=False))
    return b"".join(out) + (bc.EOF_BLOCK if eof else b"")


def write_variants(d, texts, seed=0, lo=1, hi=4000, tag=""):
    """{"plain" / "bgzf" / "gzip": {file name: path}} of the texts {file name: bytes}: the BGZF copies with seeded block sizes, different ones per file"""
    out = {"plain": {}, "bgzf": {}, "gzip": {}}
    for k, (fn, text) in enumerate(sorted(texts.items())):
        for kind, data in (("plain", text), ("bgzf", bgzf(text, seeded_sizes(len(text), seed + 17 * k, lo, hi))), ("gzip", gzip.compress(text))):
            p = os.path.join(str(d), tag + fn + {"plain": "", "bgzf": ".bgz.gz", "gzip": ".gz"}[kind])
            with open(p, "wb") as f:
                f.write(data)
            out[kind][fn] = p
    return out


def damaged(blob, k):
    """the chain `blob` with its block k damaged in the ways of bgzf_cases.bad_block_files() -> [(name, bytes)]: footer CRC flipped, ISIZE one
    lower, ISIZE one higher, a payload byte zeroed.  The chain itself stays whole (every BSIZE is as it was)."""
    off, size, pay, n_pay, crc, isize = bc.members(blob)[k]
    assert 0 < (isize & 255) < 255 and n_pay > 8
    out = []
    for name, at, v in (("crc", off + size - 8, blob[off + size - 8] ^ 1), ("isize-1", off + size - 4, (isize - 1) & 255), ("isize+1", off + size - 4, (isize + 1) & 255)):
        b = bytearray(blob)
        b[at] = v
        out.append((name, bytes(b)))
    b = bytearray(blob)
    at = next(i for i in range(pay + n_pay // 2, pay + n_pay) if b[i] != 0)
    b[at] = 0
    out.append(("payload", bytes(b)))
    return out


def block_offset(blob, k):
    """(file offset of member k, file offset of its deflate stream)"""
    m = bc.members(blob)[k]
    return m[0], m[2]


def stderr_lines(err):
    """stderr without the footer and the timing lines (and without what the sanitized build says about the buffers a run that ends in
    exit(EXIT_FAILURE) leaves allocated, as the reference does)"""
    text = err.decode(errors="replace").split("\n=================================================================")[0]
    return [ln for ln in text.splitlines() if not ln.startswith("[main]") and " seconds" not in ln and ln.strip()]


def per_base(contigs):
    """[(name, [depth, ...])] -> per-base bedgraph text"""
    return b"".join(b"%s\t%d\t%d\t%d\n" % (name, p, p + 1, v) for name, vals in contigs for p, v in enumerate(vals))


