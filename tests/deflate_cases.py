"""The payloads of the BGZF encoder's tests (csrc/deflate.hpp: on the CPU in tests/test_deflate_host.py, on the device in
tests/test_gpu_deflate.py), each the smallest shape at which the encoder can still go wrong, and the checks both share: zlib is the
reference throughout."""
import random
import struct
import zlib

import bgzf_cases as bc

MEMBER = 65280           # payload bytes of a member (CND_MEMBER)
MAX_SIZE = 65311         # MEMBER + 5 (stored block) + 26 (header and footer)


def fastq_like(n, seed):
    """names, bases, '+', qualities: reads of a few hundred to a few thousand bases until n bytes are there"""
    rng = random.Random(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        ln = rng.randrange(200, 3000)
        out += b"@%08x-%04x-read%d\n" % (rng.getrandbits(32), rng.getrandbits(16), k)
        out += bytes(rng.choice(b"ACGT") for _ in range(ln)) + b"\n+\n"
        out += bytes(33 + min(50, max(2, int(rng.gauss(28, 9)))) for _ in range(ln)) + b"\n"
        k += 1
    return bytes(out[:n])


def fibonacci_block(with_eob=False):
    """22 symbols with the counts 1, 1, 2, 3, 5, ... 17711: 46367 bytes, shuffled; their unlimited Huffman tree is 21 deep.  with_eob: without
    the first symbol — the counts are those numbers together with the block's one end-of-block symbol, whose tree an encoder really builds
    (a third count of 1 lets the tree above branch into two chains of half the depth)"""
    counts = [1, 1]
    while len(counts) < 22:
        counts.append(counts[-1] + counts[-2])
    assert sum(counts) == 46367 and counts[-1] == 17711
    data = bytearray()
    for k, c in enumerate(counts[1:] if with_eob else counts):
        data += bytes([65 + k]) * c
    random.Random(22).shuffle(data)
    return bytes(data)


def huffman_depth(counts):
    """the depth of the Huffman tree of the counts (two lightest first, a leaf before a node of the same weight)"""
    heap = sorted((c, 0, 0) for c in counts)
    k = 0
    while len(heap) > 1:
        (a, _, da), (b, _, db) = heap[0], heap[1]
        k += 1
        heap = sorted(heap[2:] + [(a + b, k, max(da, db) + 1)])
    return heap[0][2]


def _runs(lengths, seed):
    """runs of the given lengths of one value each, a different byte between two of them"""
    rng = random.Random(seed)
    out = bytearray()
    for i, ln in enumerate(lengths):
        out += bytes([65 + i % 20]) * ln + bytes([97 + rng.randrange(26)])
    return bytes(out)


def _run_at(start):
    """a run of 4 that begins at byte `start` of the second tile; no other byte equals the one in front of it"""
    body = bytearray(b"ACGT"[i % 4] for i in range(64 + start))
    body += b"N" * 4
    body += bytearray(b"TGCA"[i % 4] for i in range(70))
    return bytes(body)


def quality_less_record(n):
    return b"@read-without-qualities\n" + bc.acgt(n, 5, width=10 ** 9)[:n] + b"\n+\n" + b'"' * n + b"\n"


def payloads():
    """name -> (bytes of the text, offset at which the source range begins)"""
    p = {}
    for n in (0, 1, 2, 63, 64, 65, MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER):
        p["len_%d" % n] = (fastq_like(n, n + 1), 0)
    p["one_value"] = (b"G" * MEMBER, 0)
    p["all_256"] = (bytes(range(256)), 0)
    rng = random.Random(4)
    p["acgt"] = (bytes(rng.choice(b"ACGT") for _ in range(MEMBER)), 0)
    p["fastq"] = (fastq_like(MEMBER, 99), 0)
    p["random"] = (bc.rand_bytes(MEMBER, 8), 0)
    p["fibonacci"] = (fibonacci_block(), 0)
    p["fibonacci_eob"] = (fibonacci_block(True), 0)
    p["runs"] = (_runs([3, 4, 5, 258, 259, 260, 261, 262, 516, 517, 520], 3), 0)
    for s in (61, 62, 63, 64):
        p["run4_at_%d" % s] = (_run_at(s), 0)
    p["run_over_the_cut"] = (b"xy" + b"T" * (MEMBER + 1) + b"z", 0)
    p["no_qualities"] = (quality_less_record(3001), 0)
    p["odd_offset"] = (b"#" * 4097 + fastq_like(70001, 5), 4097)
    return p


def check_chain(blob, payload):
    """the BGZF chain `blob` (no end-of-file block) is the members of `payload` cut every MEMBER bytes: under zlib's raw inflate every member
    is its piece, with the piece's CRC-32 and ISIZE and a size of at most MAX_SIZE -> the members' sizes"""
    rows = bc.members(blob)
    assert len(rows) == (len(payload) + MEMBER - 1) // MEMBER, (len(rows), len(payload))
    sizes, at = [], 0
    for k, (off, size, pay, n_pay, crc, isize) in enumerate(rows):
        assert off == at and size <= MAX_SIZE, (k, off, size)
        piece = payload[k * MEMBER:(k + 1) * MEMBER]
        z = zlib.decompressobj(-15)
        got = z.decompress(blob[pay:pay + n_pay]) + z.flush()
        assert z.eof and z.unused_data == b"" and got == piece, (k, len(got), len(piece))
        assert isize == len(piece) and crc == zlib.crc32(piece), k
        assert struct.unpack_from("<H", blob, off + 16)[0] == size - 1
        sizes.append(size)
        at += size
    assert at == len(blob)
    return sizes


def check_sizes(name, sizes, payload):
    """the size conditions of the encoder"""
    if name == "one_value":
        assert sizes[0] <= 512, sizes
    if name == "acgt":
        assert sizes[0] <= 19000, sizes
    if name == "fastq":
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        assert sizes[0] <= len(z.compress(payload) + z.flush()) + 26, sizes
    if name == "random":
        assert sizes[0] == MAX_SIZE, sizes
