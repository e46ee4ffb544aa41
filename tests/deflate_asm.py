"""A deflate assembler (CPU, pure Python): streams put together token by token, so that the decoder of csrc/inflate.hpp meets what zlib's
inflate accepts and zlib's deflate never writes — maximal-width tokens, codes deeper than the primary tables used by matches, code-length
runs across the literal/distance boundary (as libdeflate writes them), the incomplete code sets inflate_table() allows, empty stored
blocks at every bit alignment — and, on the device, matches and literal runs at every position against the 64 lanes and the lazy fence.
valid_cases() / invalid_cases() are the material of tests/test_deflate_asm_host.py (zlib and the sanitizer program) and of
tests/test_gpu_inflate_crafted.py.  Nothing here calls zlib's deflate; the expected bytes come from expand().  No data byte is 0xA5, the
value the device test fills its output with.

Two shapes that a BGZF member cannot hold are replaced by their nearest neighbours: a dynamic block with HCLEN = 4 has code lengths for
16, 17, 18 and 0 alone, so that every literal/length length is 0 and the end-of-block code is missing (it is an invalid case here, and the
smallest valid HCLEN, 5, is the valid one); and a stored block of 65535 bytes is larger than the 65510 bytes of payload a member of 64 KiB
has room for (the largest that fits, 65505 bytes, is the valid case; LEN = 65535 is read in an invalid one)."""
import random
import struct
import zlib

from bgzf_cases import _DBASE, _DEXT, _LBASE, _LEXT, _ORDER

FILL = 0xA5
ALPHA = [c for c in range(256) if c != FILL]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
BAD_BLOCK, BAD_CODES, BAD_SYMBOL, BAD_DISTANCE, BAD_LENGTH, BAD_INPUT = 1, 2, 3, 4, 5, 6      # the CNI_BAD_* of csrc/inflate.hpp
LEN_EDGES = [3, 4, 63, 64, 65, 66, 128, 129, 257, 258]


def len_sym(n):
    """the canonical length symbol of a match of n bytes"""
    assert 3 <= n <= 258
    return 285 if n == 258 else 257 + max(i for i in range(28) if _LBASE[i] <= n)


def dist_sym(d):
    assert 1 <= d <= 32768
    return max(i for i in range(30) if _DBASE[i] <= d)


def canon(lens):
    """{symbol: (code, length)} of the canonical code"""
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
            tab[s] = (nxt[x], x)
            nxt[x] += 1
    return tab


def kraft(lens):
    """the code space the lengths take, in units of 2^-15: 32768 is a complete set"""
    return sum(1 << (15 - x) for x in lens if x)


def flat(n):
    """n code lengths of a complete set, as equal as they can be"""
    if n < 2:
        return [1] * n
    k = (n - 1).bit_length()
    return [k - 1] * ((1 << k) - n) + [k] * (2 * n - (1 << k))


def rand_complete(n, rng, cap=15):
    """n code lengths of a complete set with no length above cap: a random binary tree, leaf by leaf"""
    if n < 2:
        return [1] * n
    assert n <= 1 << cap
    leaves = [1, 1]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < cap]
        i = rng.choice(open_)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return leaves


def complete(want, size, fillers=()):
    """the code lengths of symbols 0 .. size - 1: want {symbol: length} as it is, and what is left of the code space handed to the symbols of
    `fillers`, largest piece first, so that the set is complete"""
    lens = [0] * size
    for s, x in want.items():
        lens[s] = x
    left, fillers = 32768 - kraft(lens), [s for s in fillers if s not in want]
    assert left >= 0
    while left:
        piece = 1 << (left.bit_length() - 1)
        lens[fillers.pop(0)] = 15 - (piece.bit_length() - 1)
        left -= piece
    return lens


def spread(symbols, lengths, size):
    lens = [0] * size
    for s, x in zip(symbols, lengths):
        lens[s] = x
    assert len(symbols) == len(lengths)
    return lens


def _apply(out, tokens):
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t[0], t[1]
            assert 1 <= d <= len(out)
            for _ in range(n):
                out.append(out[-d])


def expand(tokens, before=b""):
    """the bytes the tokens stand for behind the bytes `before`"""
    out = bytearray(before)
    _apply(out, tokens)
    return bytes(out[len(before):])


def unrun(cl_syms):
    """the code lengths a sequence of (code-length symbol, extra bits) stands for"""
    lens = []
    for s, e in cl_syms:
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + e)
        elif s == 17:
            lens += [0] * (3 + e)
        else:
            lens += [0] * (11 + e)
    return lens


def plain(lens):
    return [(x, 0) for x in lens]


def rle(lens, rng):
    """the combined length array run-length-coded with seeded choices: runs of 16, 17 and 18 of random counts wherever one fits, across
    the boundary between the two sets as anywhere else"""
    out, i = [], 0
    while i < len(lens):
        r = 1
        while i + r < len(lens) and lens[i + r] == lens[i]:
            r += 1
        if lens[i] == 0 and r >= 3 and rng.random() < 0.8:
            if r >= 11 and rng.random() < 0.7:
                k = rng.randint(11, min(r, 138))
                out.append((18, k - 11))
            else:
                k = rng.randint(3, min(r, 10))
                out.append((17, k - 3))
            i += k
        elif i > 0 and lens[i] == lens[i - 1] and r >= 3 and rng.random() < 0.8:
            k = rng.randint(3, min(r, 6))
            out.append((16, k - 3))
            i += k
        else:
            out.append((lens[i], 0))
            i += 1
    return out


class Asm:
    """a bit writer (deflate's order: the low bit first, Huffman codes from their high bit) with the three block emitters; .out collects the
    bytes the stream stands for"""

    def __init__(self):
        self.buf, self.acc, self.n, self.out = bytearray(), 0, 0, bytearray()

    @property
    def pos(self):
        return 8 * len(self.buf) + self.n

    def bits(self, v, k):
        """the raw escape: k bits of v"""
        assert 0 <= v < (1 << k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        v, k = c
        self.bits(int(format(v, "0%db" % k)[::-1], 2), k)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.buf)

    def stored(self, data, last=False, length=None, nlen=None):
        self.bits(int(last), 1)
        self.bits(0, 2)
        self.align()
        length = len(data) if length is None else length
        self.bits(length, 16)
        self.bits(length ^ 0xFFFF if nlen is None else nlen, 16)
        self.buf += data
        self.out += data

    def tokens(self, tokens, lc, dc):
        for t in tokens:
            if isinstance(t, int):
                self.code(lc[t])
            else:
                n, d = t[0], t[1]
                s = t[2] if len(t) > 2 else len_sym(n)
                assert 0 <= n - _LBASE[s - 257] < (1 << _LEXT[s - 257]) or n == _LBASE[s - 257]
                self.code(lc[s])
                self.bits(n - _LBASE[s - 257], _LEXT[s - 257])
                ds = dist_sym(d)
                self.code(dc[ds])
                self.bits(d - _DBASE[ds], _DEXT[ds])
        _apply(self.out, tokens)

    def fixed(self, tokens, last=False, eob=True):
        self.bits(int(last), 1)
        self.bits(1, 2)
        lc = canon(FIXED_LIT)
        self.tokens(tokens, lc, canon(FIXED_DIST))
        if eob:
            self.code(lc[256])

    def dyn_head(self, hlit, hdist, cl_lens, hclen=None, last=False):
        """the header of a dynamic block up to the code-length code lengths; hlit and hdist are the counts (257 .., 1 ..), unchecked"""
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[_ORDER[i]]])
        assert all(cl_lens[_ORDER[i]] == 0 for i in range(hclen, 19))
        self.bits(int(last), 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[_ORDER[i]], 3)

    def cl_run(self, cl_syms, cl_lens):
        cc = canon(cl_lens)
        for s, e in cl_syms:
            self.code(cc[s])
            if s >= 16:
                self.bits(e, {16: 2, 17: 3, 18: 7}[s])

    def dynamic(self, lit_lens, dist_lens, tokens, last=False, cl_syms=None, cl_lens=None, hclen=None, check=True, eob=True):
        """lit_lens: HLIT code lengths, dist_lens: HDIST of them; cl_syms: the (code-length symbol, extra bits) sequence that sends them, by
        default a symbol per length; cl_lens: the 19 lengths of the code-length code, by default a flat set over the symbols cl_syms uses;
        check=False lets lengths and runs through that are not a valid block"""
        seq = list(lit_lens) + list(dist_lens)
        if cl_syms is None:
            cl_syms = plain(seq)
        if cl_lens is None:
            used = sorted({s for s, _ in cl_syms})
            if len(used) < 2:
                used = sorted(set(used) | {0, 18})[:2]
            cl_lens = spread(used, flat(len(used)), 19)
        if check:
            assert unrun(cl_syms) == seq and 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30 and lit_lens[256]
            assert kraft(cl_lens) == 32768 and max(cl_lens) <= 7
            for ls, n in ((lit_lens, 286), (dist_lens, 30)):
                assert kraft(ls) == 32768 or sum(x > 0 for x in ls) <= 1 and max(ls) <= 1, ls
        self.dyn_head(len(lit_lens), len(dist_lens), cl_lens, hclen, last)
        self.cl_run(cl_syms, cl_lens)
        lc = canon(lit_lens)
        self.tokens(tokens, lc, canon(dist_lens))
        if eob:
            self.code(lc[256])


def member_raw(payload, data=None, isize=None, crc=None):
    """one BGZF member around a deflate stream made elsewhere; the footer is that of `data`, or as given"""
    if data is not None:
        isize, crc = len(data), zlib.crc32(data) & 0xFFFFFFFF
    bsize = 18 + len(payload) + 8 - 1
    assert bsize <= 0xFFFF and isize <= 65536, (bsize, isize)
    return struct.pack("<4BIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, bsize) + payload + struct.pack("<II", crc or 0, isize)


def lens_for(tokens, rng=None, spare_lit=0, spare_dist=0):
    """complete literal/length and distance code lengths for the tokens (and the end-of-block code): flat, or a seeded random tree with
    `spare` symbols more than the tokens use"""
    lits, dists = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(t[2] if len(t) > 2 else len_sym(t[0]))
            dists.add(dist_sym(t[1]))
    if rng is not None:
        free = [s for s in range(286) if s not in lits and s != FILL]
        lits |= set(rng.sample(free, min(spare_lit, len(free))))
        free = [s for s in range(30) if s not in dists]
        dists |= set(rng.sample(free, min(spare_dist, len(free))))
    lits, dists = sorted(lits), sorted(dists)
    ll = rand_complete(len(lits), rng) if rng is not None else flat(len(lits))
    dl = rand_complete(len(dists), rng) if rng is not None else flat(len(dists))
    return spread(lits, ll, max(257, lits[-1] + 1)), spread(dists, dl, dists[-1] + 1 if dists else 1)


def text(n, seed, alphabet=None):
    r = random.Random(seed)
    a = alphabet or ALPHA
    return [r.choice(a) for _ in range(n)]


# ---- the valid cases ----------------------------------------------------------------------------------------------------------------------
def _max_token():
    # 16 literal/length codes of 1 .. 14, 15, 15 bits: length symbol 284 and one literal take the two 15-bit codes; the same for the distances
    lit_syms = [0x41 + i for i in range(13)] + [256, 0x5A, 284]            # 'A' .. 'M': 1 .. 13 bits, end-of-block: 14, 'Z' and 284: 15
    ll = spread(lit_syms, list(range(1, 15)) + [15, 15], 285)
    dl = spread(list(range(14)) + [28, 29], list(range(1, 15)) + [15, 15], 30)
    big = (258, 32768, 284)                                                  # 15 + 5 + 15 + 13 bits
    toks = text(32768, 31, [0x41, 0x41, 0x41, 0x42, 0x42, 0x43, 0x44, 0x45])
    toks += [big, 0x5A, big, big, big]
    for k in range(24):          # the token begins at every offset against the 56 to 63 bits a refill leaves
        toks += [0x41] * k + [big]
    a = Asm()
    a.dynamic(ll, dl, toks, last=True)
    return a, lambda w: w["max_token_bits"] == 48 and w["max_code_len"] == 15 and w["matches"] == 28 and w["hclen"] == [19]


def _dist_walk():
    dl = spread(range(16), list(range(1, 15)) + [15, 15], 16)
    toks = text(300, 32)
    for ds in range(8, 16):       # distance symbols 8 .. 15: codes of 9 .. 15 bits, behind the 8 bits of the primary table
        toks += [(5 + ds, _DBASE[ds] + ds % (1 << _DEXT[ds])), ALPHA[ds]]
    ll, _ = lens_for(toks)
    a = Asm()
    a.dynamic(ll, dl, toks, last=True)
    return a, lambda w: set(range(9, 16)) <= w["dist_code_lens"]


def _len_walk():
    lits = [0x61 + i for i in range(9)]
    lit_syms = lits + [256] + [257, 260, 265, 270, 280, 285]               # the length symbols: codes of 11 .. 15 bits
    ll = spread(lit_syms, list(range(1, 15)) + [15, 15], 286)
    toks = text(100, 33, lits)
    for s in (257, 260, 265, 270, 280, 285):
        n = _LBASE[s - 257] + (1 << _LEXT[s - 257]) - 1 if s != 285 else 258
        toks += [(n, 7 + s % 5), lits[s % 9]]
    _, dl = lens_for(toks)
    a = Asm()
    a.dynamic(ll, dl, toks, last=True)
    return a, lambda w: set(range(11, 16)) <= w["len_code_lens"] and w["max_len"] == 258


def _run_over_hlit(code):
    if code == 16:
        # literal/length: 'a', 'b': 4 bits, end-of-block: 3, 257 .. 259: 2; distances 0 .. 3: 2 -- the run of six 2s covers 258, 259 and all four
        ll = spread([0x61, 0x62, 256, 257, 258, 259], [4, 4, 3, 2, 2, 2], 260)
        dl = [2, 2, 2, 2]
        cl = plain(ll[:258]) + [(16, 3)]
        toks = [0x61, 0x62, 0x62, 0x61, (3, 1), (4, 2), 0x61, (5, 3), (4, 4), 0x62, (3, 4)]
    elif code == 17:
        # 258, 259 without a code, and distances 0 .. 2 without one: a run of five zeros; distances 3 and 4 have the codes
        ll = spread([0x61, 0x62, 256, 257], [2, 2, 2, 2], 260)
        dl = [0, 0, 0, 1, 1]
        cl = plain(ll[:258]) + [(17, 2)] + plain(dl[3:])
        toks = [0x61, 0x62, 0x62, 0x61, 0x61, 0x62, (3, 4), (3, 5), 0x61, (3, 6), (3, 4)]
    else:
        # 262 .. 269 without a code and distances 0 .. 4: thirteen zeros; distances 5 and 6 have the codes
        ll = spread([0x61, 0x62, 256, 261], [2, 2, 2, 2], 270)
        dl = [0, 0, 0, 0, 0, 1, 1]
        cl = plain(ll[:262]) + [(18, 2)] + plain(dl[5:])
        toks = text(12, 34, [0x61, 0x62]) + [(7, 7), (7, 8), 0x61, (7, 9), (7, 12)]
    a = Asm()
    a.dynamic(ll, dl, toks, last=True, cl_syms=cl)
    return a, lambda w: w["run_over_hlit"] == {code} and w["matches"] >= 4 and w["n_dist_codes"] == [sum(x > 0 for x in dl)]


def _one_dist_code():
    toks = text(5, 35) + [(3, 1), 0x30, (258, 1), 0x31, (64, 1), (65, 1)]
    ll, _ = lens_for(toks)
    a = Asm()
    a.dynamic(ll, [1], toks, last=True)
    return a, lambda w: w["n_dist_codes"] == [1] and w["hdist"] == [1] and w["max_dist"] == 1 and w["matches"] == 4


def _no_dist_code():
    toks = text(200, 36)
    ll, _ = lens_for(toks)
    a = Asm()
    a.dynamic(ll, [0], toks, last=True)
    return a, lambda w: w["n_dist_codes"] == [0] and w["hdist"] == [1] and w["out"] == 200


def _only_eob():
    only = spread([256], [1], 257)
    a = Asm()
    a.fixed(text(70, 37))
    a.dynamic(only, [0], [], cl_syms=[(18, 127), (18, 107), (1, 0), (0, 0)])       # 138 + 118 zeros, the 1, the distance length
    a.fixed([(5, 70)] + text(3, 38))
    a.dynamic(only, [0], [], last=True)
    return a, lambda w: w["kinds"] == ["fixed", "dynamic", "fixed", "dynamic"] and w["n_lit_codes"] == [1, 1] and w["out"] == 78


def _hlit286_hdist30():
    ll, dl = flat(286), flat(30)
    toks = text(30000, 39, ALPHA[:64]) + [(258, 400), 0x33, (258, 24577), (3, 29999), 0x34, (17, 30000)]
    a = Asm()
    a.dynamic(ll, dl, toks, last=True)
    return a, lambda w: w["hlit"] == [286] and w["hdist"] == [30] and w["n_lit_codes"] == [286] and w["n_dist_codes"] == [30] and {285} <= w["len_syms"] and {29} <= w["dist_syms"]


def _hclen_5():
    # code lengths for 16, 17, 18, 0 and 8 alone: 256 literal/length codes of 8 bits (1 .. 256), no distance code
    ll = [0] + [8] * 256
    toks = text(100, 40, [c for c in ALPHA if c])
    a = Asm()
    a.dynamic(ll, [0], toks, last=True, cl_syms=[(0, 0), (8, 0)] + [(16, 3)] * 42 + [(16, 0), (0, 0)], cl_lens=spread([16, 0, 8], [1, 2, 2], 19))
    return a, lambda w: w["hclen"] == [5] and w["code16"] and w["out"] == 100


def _hclen_19():
    # the last of the 19 code-length code lengths is that of 15
    toks = text(50, 41, [0x41, 0x42, 0x43]) + [(9, 1)]
    ll = complete({0x41: 1, 0x42: 2, 0x43: 3, 256: 5, 263: 15}, 264, fillers=range(0x50, 0x70))
    a = Asm()
    a.dynamic(ll, [1], toks, last=True)
    return a, lambda w: w["hclen"] == [19] and w["max_code_len"] == 15


def _len258_as_284():
    toks = text(9, 42) + [(258, 9, 284), 0x35, (258, 1, 284), (258, 258, 284)]
    a = Asm()
    a.fixed(toks[:11])
    ll, dl = lens_for(toks[11:])
    a.dynamic(ll, dl, toks[11:], last=True)
    return a, lambda w: w["len_syms"] == {284} and w["max_len"] == 258 and w["matches"] == 3


def _sync_flush(k):
    # a fixed block of n8 8-bit and n9 9-bit literals takes 10 + 8 n8 + 9 n9 bits: the next header begins at bit (2 + n9) % 8
    n9 = (k - 2) % 8
    a = Asm()
    a.fixed(text(20, 43 + k, ALPHA[:100]) + text(n9, 60 + k, [c for c in ALPHA if c >= 144]))
    assert a.pos % 8 == k
    a.stored(b"")
    a.fixed([(20 + n9, 20 + n9), 0x36, (4, 3)])
    a.stored(b"")
    a.stored(b"", last=True)
    return a, lambda w: w["empty_stored"][0] == k and len(w["empty_stored"]) == 3 and w["matches"] == 2


def _stored_edges():
    a = Asm()
    a.fixed(text(3, 70))
    for i, n in enumerate((0, 1, 63, 64, 65)):
        while ((a.pos + 10) // 8 + 4) % 2 == 0:     # blocks of one literal, 18 bits each, until the stored bytes begin at an odd offset
            a.fixed(text(1, 80 + a.pos))
        a.stored(bytes(text(n, 71 + i)))
        a.fixed(text(1 + i % 2, 80 + i))
    a.stored(bytes(text(100, 90)))
    a.fixed([(100, 100), (3, 1), (64, 203)])       # out of the stored block, and over the seam of both
    a.stored(bytes(text(65, 91)), last=True)
    return a, lambda w: w["stored"] == [0, 1, 63, 64, 65, 100, 65] and all(at % 2 for at in w["stored_at"][:5]) and w["kinds"][-1] == "stored" and w["end"] == 8 * len(a.buf)


def _stored_max():
    # the largest stored block a BGZF member has room for, as the only and final block: it ends with n_src
    a = Asm()
    a.stored(bytes(text(65505, 92)), last=True)
    return a, lambda w: w["stored"] == [65505] and w["end"] == 8 * 65510


def _tiny_blocks():
    r = random.Random(93)
    a = Asm()
    for i in range(200):
        toks = [r.choice(ALPHA) for _ in range(1 + i % 3)]
        if i % 2:
            ll, dl = lens_for(toks, r, spare_lit=r.randint(0, 3))
            a.dynamic(ll, dl, toks, last=i == 199, cl_syms=rle(ll + dl, r))
        else:
            a.fixed(toks)
    return a, lambda w: w["kinds"] == ["fixed", "dynamic"] * 100 and w["out"] == sum(1 + i % 3 for i in range(200)) and w["matches"] == 0


def _fence_grid():
    out = {}
    for k in (0, 1, 63, 64, 65):
        for where in ("out1", "out1+1", "out1+3", "out"):
            toks = ALPHA[10:80] + [(3, 70)]          # out1 = 70: the bytes behind it are the first match's
            toks += text(k, 94 + k)
            now = 73 + k
            end = {"out1": 70, "out1+1": 71, "out1+3": 73, "out": now}[where]
            toks += [(3, now - end + 3), (10, 2), 0x37]
            a = Asm()
            a.fixed(toks, last=True)
            out["fence_grid/k%d_%s" % (k, where)] = (a, lambda w, n=now + 14: w["out"] == n and w["matches"] == 3 and w["overlaps"] == 1)
    return out


def _copy_grid():
    out, i = {}, 0
    for p in (1, 63, 64, 65, 130):
        for n in LEN_EDGES:
            for d in sorted({1, 2, 3, 63, 64, 65, n - 1, n, n + 1, p}):
                if not 1 <= d <= p:
                    continue
                toks = text(p, 1000 + i) + [(n, d), 0x38]
                a = Asm()
                if i % 2:
                    a.fixed(toks, last=True)
                else:
                    ll, dl = lens_for(toks)
                    a.dynamic(ll, dl, toks, last=True)
                out["copy_grid/p%d_len%d_dist%d" % (p, n, d)] = (a, lambda w, p=p, n=n, d=d: w["out"] == p + n + 1 and w["max_len"] == n and w["max_dist"] == d)
                i += 1
    # exact_end: 65536 bytes, the last of them the last byte of a match
    toks = text(262, 95) + [(258, 262 - j % 7) for j in range(253)]
    a = Asm()
    ll, dl = lens_for(toks)
    a.dynamic(ll, dl, toks, last=True)
    out["copy_grid/exact_end"] = (a, lambda w: w["out"] == 65536 and w["matches"] == 253)
    return out


def _seeded(seed=20240917, n_members=300):
    """every stream is valid by construction: distances never exceed what is out, lengths never what is left of the member's 4096 bytes,
    every code set is a complete tree (or the single code / no code inflate allows), every run-length sequence expands to the lengths"""
    r = random.Random(seed)
    out = {}
    for m in range(n_members):
        a, room = Asm(), r.randint(0, 4096)
        n_blocks = r.randint(1, 4)
        for blk in range(n_blocks):
            last = blk == n_blocks - 1
            kind = r.choice(("stored", "fixed", "dynamic", "dynamic"))
            left = room - len(a.out)
            if kind == "stored":
                a.stored(bytes(r.choice(ALPHA) for _ in range(r.choice((0, 1, 63, 64, 65, left // 2, left)) if left else 0))[:left], last)
                continue
            toks, now = [], len(a.out)
            for _ in range(r.randint(0, 40)):
                left = room - now
                lens = [x for x in LEN_EDGES + [r.randint(3, 258)] if x <= left]
                if now and lens and r.random() < 0.5:
                    n = r.choice(lens)
                    d = r.choice([x for x in (1, 2, 3, 63, 64, 65, n - 1, n, n + 1, now, r.randint(1, now)) if 1 <= x <= now])
                    toks.append((n, d, 284) if n == 258 and r.random() < 0.3 else (n, d))
                    now += n
                elif left:
                    run = [r.choice(ALPHA) for _ in range(min(left, r.choice((1, 1, 2, 63, 64, 65))))]
                    toks += run
                    now += len(run)
            if kind == "fixed":
                a.fixed(toks, last)
            else:
                ll, dl = lens_for(toks, r, spare_lit=r.randint(0, 20), spare_dist=r.randint(0, 6))
                ll += [0] * r.randint(0, 286 - len(ll)) if r.random() < 0.5 else []
                dl += [0] * r.randint(0, 30 - len(dl)) if r.random() < 0.5 else []
                cl = rle(ll + dl, r)
                used = sorted({s for s, _ in cl})
                if len(used) < 2:
                    used = sorted(set(used) | {0, 18})[:2]
                a.dynamic(ll, dl, toks, last, cl_syms=cl, cl_lens=spread(used, rand_complete(len(used), r, 7), 19))
        out["seeded/%03d" % m] = (a, lambda w, n=len(a.out), k=n_blocks: w["out"] == n and len(w["kinds"]) == k)
    return out


GROUPS = ("fence_grid", "copy_grid", "seeded")
_VALID = None


def valid_cases():
    """{name: (payload, expected bytes, check of bgzf_cases.walk()'s result)}: one BGZF member each; the names of the grids' members begin
    with the grid's name and a slash"""
    global _VALID
    if _VALID is None:
        made = {"max_token": _max_token(), "dist_walk": _dist_walk(), "len_walk": _len_walk(), "one_dist_code": _one_dist_code(), "no_dist_code": _no_dist_code(),
                "only_eob": _only_eob(), "hlit286_hdist30": _hlit286_hdist30(), "hclen_5": _hclen_5(), "hclen_19": _hclen_19(), "len258_as_284": _len258_as_284(),
                "stored_edges": _stored_edges(), "stored_max": _stored_max(), "tiny_blocks": _tiny_blocks()}
        for code in (16, 17, 18):
            made["run_over_hlit_%d" % code] = _run_over_hlit(code)
        for k in range(8):
            made["sync_flush_%d" % k] = _sync_flush(k)
        made.update(_fence_grid())
        made.update(_copy_grid())
        made.update(_seeded())
        _VALID = {}
        for name, (a, check) in made.items():
            assert FILL not in a.out and len(a.out) <= 65536, name
            _VALID[name] = (a.done(), bytes(a.out), check)
    return _VALID


def singles():
    return sorted(n for n in valid_cases() if "/" not in n and n != "tiny_blocks")


def group(name):
    return sorted(n for n in valid_cases() if n.startswith(name + "/"))


# ---- the invalid cases --------------------------------------------------------------------------------------------------------------------
def _cut_inside(a, begin, end):
    """the stream cut at a byte boundary inside the bits [begin, end)"""
    n = (begin + 8) // 8
    assert begin < 8 * n < end
    return a.done()[:n]


def invalid_cases():
    """{name: (payload, n_dst, the CNI_BAD_* reason csrc/inflate.hpp gives)}"""
    out = {}
    lits = [0x61, 0x62, 0x63]
    ll4 = spread(lits + [256], [2, 2, 2, 2], 257)               # a complete literal set of four codes
    cl3 = spread([0, 1, 2, 18], [2, 2, 2, 2], 19)

    a = Asm()
    a.bits(1, 1), a.bits(3, 2), a.bits(0, 13)
    out["block_type_3"] = (a.done(), 16, BAD_BLOCK)

    a = Asm()
    a.stored(b"abcdefgh", last=True, nlen=8 ^ 0xFFFE)
    out["len_nlen_mismatch"] = (a.done(), 8, BAD_BLOCK)

    a = Asm()
    a.stored(b"abcdefgh", last=True, length=65535)              # LEN = 0xFFFF, NLEN = 0, eight bytes there
    out["stored_past_the_input"] = (a.done(), 65535, BAD_INPUT)
    a = Asm()
    a.fixed([0x61, 0x62])
    a.stored(b"abcdefgh", last=True, length=9)
    out["stored_one_past_the_input"] = (a.done(), 11, BAD_INPUT)

    a = Asm()
    a.fixed([0x61, 0x62])
    a.stored(b"abcdefgh", last=True)
    out["stored_past_n_dst"] = (a.done(), 9, BAD_LENGTH)

    # the three over-subscribed sets
    a = Asm()
    a.dyn_head(257, 1, spread([0, 1, 2], [1, 1, 1], 19), last=True)
    a.bits(0, 64)
    out["oversubscribed_code_lengths"] = (a.done(), 4, BAD_CODES)
    a = Asm()
    a.dynamic(spread(lits + [256, 257], [2, 2, 2, 2, 2], 258), [0], [0x61], last=True, check=False)
    out["oversubscribed_literals"] = (a.done(), 1, BAD_CODES)
    a = Asm()
    a.dynamic(ll4, [1, 1, 1], [0x61], last=True, check=False)
    out["oversubscribed_distances"] = (a.done(), 1, BAD_CODES)

    # the incomplete ones
    a = Asm()
    a.dyn_head(257, 1, spread([0], [1], 19), last=True)          # one code-length code of one bit: allowed for the other two kinds only
    a.bits(0, 300)
    out["incomplete_code_lengths"] = (a.done(), 0, BAD_CODES)
    a = Asm()
    a.dynamic(spread(lits[:2] + [256], [2, 2, 2], 257), [0], [0x61], last=True, check=False)
    out["incomplete_literals"] = (a.done(), 1, BAD_CODES)
    a = Asm()
    a.dynamic(spread([256], [2], 257), [0], [], last=True, check=False)                # one code, but of two bits
    out["incomplete_literals_one_long_code"] = (a.done(), 0, BAD_CODES)
    a = Asm()
    a.dynamic(ll4, [2, 2, 2], [0x61], last=True, check=False)
    out["incomplete_distances"] = (a.done(), 1, BAD_CODES)
    a = Asm()
    a.dynamic(ll4, [0, 2], [0x61], last=True, check=False)                             # one code, but of two bits: maxlen > 1
    out["incomplete_distances_one_long_code"] = (a.done(), 1, BAD_CODES)

    cl16 = spread([0, 2, 16, 18], [2, 2, 2, 2], 19)
    a = Asm()
    a.dyn_head(257, 1, cl16, last=True)
    a.cl_run([(16, 0)] + plain(ll4[3:]) + [(0, 0)], cl16)
    a.bits(0, 32)
    out["code_16_first"] = (a.done(), 1, BAD_CODES)

    a = Asm()
    a.dynamic(ll4, [0], [0x61], last=True, cl_syms=plain(ll4) + [(17, 0)], check=False)        # 257 + 1 lengths wanted, 257 + 3 sent
    out["repeat_past_the_lengths"] = (a.done(), 1, BAD_CODES)
    a = Asm()
    a.dyn_head(257, 1, cl3, last=True)
    a.cl_run(plain(ll4[:250]) + [(18, 0)], cl3)                                                  # 250 + 11 > 258
    a.bits(0, 32)
    out["repeat_18_past_the_lengths"] = (a.done(), 1, BAD_CODES)

    a = Asm()
    a.dynamic(spread(lits + [255], [2, 2, 2, 2], 257), [0], [0x61], last=True, check=False, eob=False)
    a.bits(0, 16)
    out["no_end_of_block_code"] = (a.done(), 1, BAD_CODES)

    for name, hlit, hdist in (("hlit_287", 287, 1), ("hlit_288", 288, 1), ("hdist_31", 257, 31), ("hdist_32", 257, 32)):
        a = Asm()
        a.dyn_head(hlit, hdist, cl3, last=True)
        a.cl_run(plain(ll4) + [(0, 0)] * (hlit - 257 + hdist), cl3)
        a.code(canon(ll4)[0x61]), a.code(canon(ll4)[256])
        out[name] = (a.done(), 1, BAD_CODES)

    # HCLEN = 4: lengths for 16, 17, 18 and 0 alone, so every code length is 0 and the end-of-block code is missing
    c4 = spread([18, 0], [1, 1], 19)
    a = Asm()
    a.dyn_head(257, 1, c4, hclen=4, last=True)
    a.cl_run([(18, 127), (18, 109)], c4)
    a.bits(0, 16)
    out["hclen_4"] = (a.done(), 0, BAD_CODES)

    out_ll = spread(lits + [256, 257], [2, 2, 3, 3, 2], 258)
    a = Asm()
    a.dynamic(out_ll, [1], [0x61, 0x62, (3, 1)], eob=False, last=True)
    a.code(canon(out_ll)[257]), a.bits(1, 1)                                # the other one-bit distance code: no symbol has it
    a.code(canon(out_ll)[256])
    out["unused_code_of_one_distance_code"] = (a.done(), 8, BAD_SYMBOL)
    a = Asm()
    a.dynamic(out_ll, [0], [0x61, 0x62], eob=False, last=True)
    a.code(canon(out_ll)[257]), a.bits(0, 1)
    a.code(canon(out_ll)[256])
    out["match_without_distance_codes"] = (a.done(), 5, BAD_SYMBOL)

    fl, fd = canon(FIXED_LIT), canon(FIXED_DIST)
    for s in (286, 287):
        a = Asm()
        a.fixed([0x61, 0x62], last=True, eob=False)
        a.code(fl[s]), a.code(fd[0]), a.code(fl[256])
        out["fixed_symbol_%d" % s] = (a.done(), 5, BAD_SYMBOL)
    for s in (30, 31):
        a = Asm()
        a.fixed([0x61, 0x62], last=True, eob=False)
        a.code(fl[257]), a.code(fd[s]), a.bits(0, 13), a.code(fl[256])
        out["fixed_distance_%d" % s] = (a.done(), 5, BAD_SYMBOL)

    for name, pre in (("distance_past_the_start_at_0", 0), ("distance_past_the_start_mid_stream", 10)):
        a = Asm()
        a.fixed(text(pre, 96), last=True, eob=False)
        a.code(fl[257]), a.code(fd[dist_sym(pre + 1)]), a.bits(pre + 1 - _DBASE[dist_sym(pre + 1)], _DEXT[dist_sym(pre + 1)]), a.code(fl[256])
        out[name] = (a.done(), pre + 3, BAD_DISTANCE)

    a = Asm()
    a.fixed(text(70, 97), last=True)
    out["one_literal_too_many"] = (a.done(), 69, BAD_LENGTH)
    a = Asm()
    a.fixed(text(70, 97) + [(66, 3)], last=True)
    out["match_one_byte_too_long"] = (a.done(), 135, BAD_LENGTH)
    a = Asm()
    a.fixed(text(70, 97) + [(66, 3)], last=True)
    out["one_byte_short"] = (a.done(), 137, BAD_LENGTH)

    # the input ends ...
    toks = text(40, 98, lits) + [(258, 30, 284)]
    ll, dl = lens_for(toks)
    a = Asm()
    a.dynamic(ll, dl, toks, last=True)
    whole = a.done()
    out["ends_in_the_header"] = (whole[:1], 298, BAD_INPUT)                # inside HLIT / HDIST / HCLEN: bits 3 .. 17
    # (behind the input the decoder reads zeros: they are code lengths of 0 until the input is found to be over, never a bad code first)
    n_head = 17 + 3 * _hclen_of(whole)
    out["ends_in_the_code_lengths"] = (whole[:(n_head + 8 * 20) // 8], 298, BAD_INPUT)
    a = Asm()
    a.fixed([0x61, 0x62], last=True, eob=False)
    begin = a.pos
    a.code(fl[200])                                                           # nine bits from bit 19 on: the third byte ends inside them
    out["ends_in_a_code"] = (_cut_inside(a, begin, a.pos), 3, BAD_INPUT)
    a = Asm()
    a.fixed([0x61, 0x62], last=True, eob=False)
    a.code(fl[257]), a.code(fd[29])
    begin = a.pos
    a.bits(0x1FFF, 13), a.code(fl[256])
    out["ends_in_the_extra_bits"] = (_cut_inside(a, begin, begin + 13), 5, BAD_INPUT)
    return out


def _hclen_of(payload):
    return 4 + ((payload[1] | payload[2] << 8) >> 5 & 15)
