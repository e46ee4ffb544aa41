"""BGZF test material (CPU): a writer on Python's zlib, a small deflate walker that tells which shapes a payload holds, and the
cases of tests/test_bgzf_host.py / tests/test_gpu_bgzf.py with the shape each of them must keep covering."""
import random
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, extra_front=b""):
    """one BGZF member holding `data` (at most 65536 bytes); extra_front: other extra subfields in front of BC"""
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    payload = c.compress(data) + c.flush()
    xlen = len(extra_front) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize <= 0xFFFF, bsize
    head = struct.pack("<4BIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra_front + b"BC" + struct.pack("<HH", 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def write(data, sizes=None, eof=True, **kw):
    """`data` as a BGZF file: blocks of 65280 bytes, or of the given sizes (the last one takes the rest)"""
    out, at = [], 0
    sizes = list(sizes) if sizes is not None else []
    while at < len(data):
        n = sizes.pop(0) if sizes else 65280
        out.append(member(data[at:at + n], **kw))
        at += n
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def members(blob):
    """[(offset, size, payload offset, payload size, crc, isize)] of a BGZF chain (the walker of the tests, independent of the library's)"""
    res, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si, slen = blob[x:x + 2], struct.unpack_from("<H", blob, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", blob, x + 4)[0]
            x += 4 + slen
        size = bsize + 1
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        res.append((at, size, at + 12 + xlen, size - 12 - xlen - 8, crc, isize))
        at += size
    return res


def inflate_members(blob):
    """zlib's bytes of every member"""
    return [zlib.decompress(blob[o:o + s], 31) for o, s, *_ in members(blob)]


# ---- a deflate walker: which shapes does a raw deflate stream hold? ---------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _codes(lens):
    """canonical codes: {(length, code): symbol}"""
    cnt = [0] * 16
    for x in lens:
        cnt[x] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, x in enumerate(lens):
        if x:
            tab[(x, nxt[x])] = s
            nxt[x] += 1
    return tab


def _sym(bits, tab):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (n, code) in tab:
            return tab[(n, code)]
    raise ValueError("no such code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def walk(payload):
    """-> dict: kinds (list of 'stored' / 'fixed' / 'dynamic', one per deflate block), max_code_len, code16 (the repeat code 16 was used),
    max_len, max_dist, overlaps (matches with distance below length), matches, out (bytes produced); and what tells hand-assembled streams
    (tests/deflate_asm.py) apart: dist_code_lens / len_code_lens (the code lengths of the distance codes and length symbols that matches
    USED), len_syms / dist_syms (the symbols they used), max_token_bits (the most bits of one length + distance token, extra bits included),
    run_over_hlit (the repeat codes whose run began in the literal/length lengths and ended in the distance lengths), hlit / hdist / hclen
    and n_dist_codes / n_lit_codes (per dynamic block; the last two count the non-zero lengths), empty_stored (the bit offsets, modulo 8,
    of the headers of stored blocks of no bytes), stored / stored_at (the sizes of the stored blocks and the offsets of their bytes), end (the bit the stream ends behind)"""
    b = _Bits(payload)
    st = {"kinds": [], "max_code_len": 0, "code16": False, "max_len": 0, "max_dist": 0, "overlaps": 0, "matches": 0, "out": 0,
          "dist_code_lens": set(), "len_code_lens": set(), "len_syms": set(), "dist_syms": set(), "max_token_bits": 0, "run_over_hlit": set(),
          "hlit": [], "hdist": [], "hclen": [], "n_dist_codes": [], "n_lit_codes": [], "empty_stored": [], "stored": [], "stored_at": []}
    last = 0
    while not last:
        head = b.pos
        last, kind = b.take(1), b.take(2)
        if kind == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.take(16)
            assert b.take(16) == n ^ 0xFFFF
            st["stored"].append(n)
            st["stored_at"].append(b.pos >> 3)
            if n == 0:
                st["empty_stored"].append(head & 7)
            b.pos += 8 * n
            st["out"] += n
            st["kinds"].append("stored")
            continue
        if kind == 1:
            ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
            dl = [5] * 32
            st["kinds"].append("fixed")
        else:
            assert kind == 2
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[_ORDER[i]] = b.take(3)
            ct, lens = _codes(cl), []
            while len(lens) < hlit + hdist:
                before = len(lens)
                s = _sym(b, ct)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    st["code16"] = True
                    lens += [lens[-1]] * (3 + b.take(2))
                elif s == 17:
                    lens += [0] * (3 + b.take(3))
                else:
                    lens += [0] * (11 + b.take(7))
                if before < hlit < len(lens):
                    st["run_over_hlit"].add(s)
            assert len(lens) == hlit + hdist
            ll, dl = lens[:hlit], lens[hlit:]
            for key, v in (("hlit", hlit), ("hdist", hdist), ("hclen", hclen), ("n_lit_codes", sum(x > 0 for x in ll)), ("n_dist_codes", sum(x > 0 for x in dl))):
                st[key].append(v)
            st["max_code_len"] = max(st["max_code_len"], max(lens))
            st["kinds"].append("dynamic")
        lt, dt = _codes(ll), _codes(dl)
        while True:
            s = _sym(b, lt)
            if s < 256:
                st["out"] += 1
            elif s == 256:
                break
            else:
                n = _LBASE[s - 257] + b.take(_LEXT[s - 257])
                ds = _sym(b, dt)
                d = _DBASE[ds] + b.take(_DEXT[ds])
                st["len_syms"].add(s)
                st["dist_syms"].add(ds)
                st["len_code_lens"].add(ll[s])
                st["dist_code_lens"].add(dl[ds])
                st["max_token_bits"] = max(st["max_token_bits"], ll[s] + _LEXT[s - 257] + dl[ds] + _DEXT[ds])
                st["matches"] += 1
                st["max_len"] = max(st["max_len"], n)
                st["max_dist"] = max(st["max_dist"], d)
                st["overlaps"] += d < n
                st["out"] += n
    st["end"] = b.pos
    return st


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def acgt(n, seed, width=60):
    r = random.Random(seed)
    s = "".join(r.choice("ACGT") for _ in range(n))
    return "\n".join(s[i:i + width] for i in range(0, len(s), width)).encode()[:n]


def rand_bytes(n, seed):
    return random.Random(seed).randbytes(n)


def _rle_data():
    return b"TTAGGG" * 5000 + acgt(4000, 5) + b"A" * 10000


def _far_data():
    head = acgt(2000, 7)
    return head + rand_bytes(30000, 8) + head + rand_bytes(28000, 9)


def skewed(n, seed):
    """n bytes of an alphabet whose counts are, with the one end-of-block symbol, the Fibonacci numbers, shuffled: the Huffman code of such
    counts is as deep as deflate allows"""
    fib = [1, 2]
    while sum(fib) < n:
        fib.append(fib[-1] + fib[-2])
    out = bytearray()
    for i, f in enumerate(fib):
        out += bytes([128 + i]) * f
    out = out[:n]
    random.Random(seed).shuffle(out)
    return bytes(out)


def cases():
    """{name: (data, member keyword arguments, check of walk()'s result)}: one BGZF member each"""
    wrapped = acgt(65000, 11)
    return {
        "stored_two": (acgt(60000, 1), dict(level=0), lambda w: w["kinds"] == ["stored", "stored"]),
        "fixed_300": (acgt(300, 2), dict(strategy=zlib.Z_FIXED), lambda w: w["kinds"] == ["fixed"]),
        "fixed_6": (b"ACGTAC", dict(strategy=zlib.Z_FIXED), lambda w: w["kinds"] == ["fixed"]),
        "level1": (wrapped, dict(level=1), lambda w: set(w["kinds"]) == {"dynamic"} and w["matches"] > 0),
        "level6": (wrapped, dict(level=6), lambda w: set(w["kinds"]) == {"dynamic"} and w["max_dist"] > 30000),
        "level9": (wrapped, dict(level=9), lambda w: set(w["kinds"]) == {"dynamic"} and w["max_dist"] > 30000),
        "huffman_only": (acgt(30000, 11), dict(strategy=zlib.Z_HUFFMAN_ONLY), lambda w: w["matches"] == 0 and len(w["kinds"]) == 2),
        "rle": (_rle_data(), dict(strategy=zlib.Z_RLE), lambda w: w["max_dist"] == 1 and w["max_len"] == 258),
        "rle_level6": (_rle_data(), dict(level=6), lambda w: w["overlaps"] > 0 and w["code16"]),
        "far": (_far_data(), dict(level=9), lambda w: w["max_dist"] >= 32000 and w["max_code_len"] >= 12 and {"dynamic", "stored"} <= set(w["kinds"])),
        # (this zlib gives the recipe above code lengths of 12 to 13, whatever the seed: the 15-bit codes have a case of their own)
        "deep_codes": (skewed(16000, 1), dict(strategy=zlib.Z_HUFFMAN_ONLY), lambda w: w["max_code_len"] == 15 and w["matches"] == 0),
        "memlevel1": (acgt(65280, 3), dict(mem_level=1), lambda w: len(w["kinds"]) >= 100),
        "isize_65536": (acgt(65536, 4), dict(level=6), lambda w: w["out"] == 65536),
        "random_stored": (rand_bytes(65280, 6), dict(level=6, mem_level=9), lambda w: w["kinds"] == ["stored", "stored"]),   # BSIZE + 1 = 65316
        "empty": (b"", dict(level=6), lambda w: w["out"] == 0),
    }


# ---- the six-block file of the bad-block tests ----------------------------------------------------------------------------------------
def six_blocks():
    text = b">s\n" + acgt(40000, 21) + b"\n>t\n" + b"TTAGGG" * 3000 + b"\n"
    return text, write(text, sizes=[9000, 1, 12000, 15000, 7000], eof=False)


def bad_block_files():
    """-> [(file bytes, n_src change of block 3)]: footer CRC flipped, ISIZE one lower, ISIZE one higher, a payload byte zeroed, n_src - 4"""
    text, blob = six_blocks()
    m = members(blob)
    assert len(m) == 6
    off, size, pay, n_pay, crc, isize = m[3]
    out = []
    for at, v in ((off + size - 8, blob[off + size - 8] ^ 1), (off + size - 4, (isize - 1) & 255), (off + size - 4, (isize + 1) & 255)):
        assert at != off + size - 4 or 0 < (isize & 255) < 255
        b = bytearray(blob)
        b[at] = v
        out.append((bytes(b), 0))
    b = bytearray(blob)
    at = next(i for i in range(pay + 40, pay + n_pay) if b[i] != 0)
    b[at] = 0
    out.append((bytes(b), 0))
    out.append((blob, -4))
    return out
