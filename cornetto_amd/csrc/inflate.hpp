// inflate.hpp — the deflate decoder, the CRC-32 and the BGZF chain walk behind cornetto_text_inflate() / cornetto_bgzf_scan(): ONE
// source for the device (inflate.hip: a wave per BGZF block) and for the CPU (tools/sim/inflate_sim.cc: the same statements with the 64
// lanes run one after the other, under the host sanitizers against zlib).  The code is written for a wave whose lanes agree on the bit
// buffer and on every symbol (the symbol loop is wave-uniform) and differ only where bytes move: in the table fill, in the literal
// gather, in the match and stored copies and in the CRC slices.  What tells the two builds apart is the lane shim S:
//   S::first(), S::step()   the lanes this thread of control runs: {lane, 64} on the device, {0, 1} on the CPU
//   S::slot(l)              where lane l keeps a per-lane value: 0 on the device (a register), l on the CPU (an array of 64)
//   S::leader()             one lane of the wave (writes of wave-uniform values to shared memory)
//   S::sync()               bytes other lanes stored (shared or global memory) are visible behind it
//   S::uni(v)               v is the same in every lane (the device build moves it to a scalar register)
// Bounds come from the code, never from the input: input is read inside [src, src + n_src) only (bits behind it read as zero, and a
// block that needed one of them is bad), output is written inside [dst, dst + n_dst) only, every loop turn consumes an input bit or
// produces an output byte, and every table index is masked or checked against the table's size.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/cornetto_accel.h"

#if defined(__HIPCC__)
#define CNI_HD __host__ __device__
#else
#define CNI_HD
#endif

#define CNI_LANES(l) for (int l = S::first(); l < 64; l += S::step())

enum {
    CNI_OK = 0,
    CNI_BAD_BLOCK = 1,     // block type 3, stored lengths that do not match, a stored block that leaves its input or output
    CNI_BAD_CODES = 2,     // over-subscribed or incomplete code set, bad repeat, too many symbols, no end-of-block code
    CNI_BAD_SYMBOL = 3,    // a code no symbol has, literal/length 286-287, distance 30-31
    CNI_BAD_DISTANCE = 4,  // a match that begins in front of the output
    CNI_BAD_LENGTH = 5,    // more or fewer bytes than n_dst
    CNI_BAD_INPUT = 6,     // bits behind the input were needed
    CNI_BAD_CRC = 7        // (bgzf_crc32) the bytes are not the footer's
};

enum { CNI_LIT_BITS = 10, CNI_DIST_BITS = 8, CNI_KIND_CODES = 0, CNI_KIND_LENS = 1, CNI_KIND_DISTS = 2 };

// per wave, in LDS on the device: 3.8 KiB
struct CniShared {
    uint16_t lit_tab[1 << CNI_LIT_BITS];     // (symbol << 4) | code length; 0: the code is longer than the index (or no code)
    uint16_t dist_tab[1 << CNI_DIST_BITS];
    uint16_t lit_sym[288], dist_sym[32], cl_sym[20];   // the symbols by code length, then by value
    uint16_t lit_cnt[16], dist_cnt[16], cl_cnt[16];    // codes of every length
    uint8_t lens[320];                       // code lengths of a dynamic block: HLIT + HDIST <= 286 + 30
    uint8_t cl_lens[20];
};

struct CniBits {
    const uint8_t *src;
    int32_t n, pos;      // pos: bytes taken into buf so far (those behind n are zeros)
    uint64_t buf;
    int32_t cnt;         // valid bits of buf
};

// at least 56 bits in the buffer
CNI_HD static inline void cni_refill(CniBits &b)
{
    if (b.pos >= 0 && b.pos <= b.n - 8) {
        uint64_t w;
        memcpy(&w, b.src + b.pos, 8);
        b.buf |= w << b.cnt;
        b.pos += (63 - b.cnt) >> 3;
        b.cnt |= 56;
        return;
    }
    while (b.cnt <= 56) {
        const uint64_t v = (b.pos >= 0 && b.pos < b.n) ? b.src[b.pos] : 0;
        b.buf |= v << b.cnt;
        b.pos += 1;
        b.cnt += 8;
    }
}
CNI_HD static inline uint32_t cni_take(CniBits &b, int k)
{
    const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1));
    b.buf >>= k;
    b.cnt -= k;
    return v;
}
// bits behind the end of the input have been consumed
CNI_HD static inline bool cni_over(const CniBits &b) { return (int64_t)b.pos * 8 - b.cnt > (int64_t)b.n * 8; }

// the canonical code that begins at the low end of `bits`, at most `maxlen` bits long -> (symbol << 4) | length, or 0
CNI_HD static inline uint32_t cni_walk(uint64_t bits, int maxlen, const uint16_t *cnt, const uint16_t *symv, int n_sym)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int c = cnt[len];
        if (code - c < first) {
            const int at = index + (code - first);
            return at < n_sym ? ((uint32_t)symv[at] << 4) | (uint32_t)len : 0;
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

// one symbol of a code through its primary table -> the symbol, or -1
template <class S>
CNI_HD static inline int cni_symbol(CniBits &b, const uint16_t *tab, int tab_bits, const uint16_t *cnt, const uint16_t *symv, int n_sym)
{
    uint32_t e = tab ? tab[b.buf & ((1u << tab_bits) - 1)] : 0;
    if (!(e & 15)) e = cni_walk(b.buf, 15, cnt, symv, n_sym);
    e = S::uni(e);
    if (!(e & 15)) return -1;
    b.buf >>= (e & 15);
    b.cnt -= (int32_t)(e & 15);
    return (int)(e >> 4);
}

// The decoding tables of lens[0 .. n): cnt[], symv[] and, if tab, the primary table of 2^tab_bits entries.  -> false: not a code set
// zlib accepts (inflate_table(): over-subscribed; incomplete unless it is a literal/length or distance set with one code of one bit, or
// a distance set without codes).
template <class S>
CNI_HD static inline bool cni_build(const uint8_t *lens, int n, int kind, uint16_t *cnt, uint16_t *symv, uint16_t *tab, int tab_bits)
{
    S::sync();                                   // lens[] is written
    CNI_LANES(l) if (l < 16) {
        int c = 0;
        for (int s = 0; s < n; ++s) c += lens[s] == l;
        cnt[l] = (uint16_t)c;
    }
    S::sync();
    int left = 1, maxlen = 0;
    for (int len = 1; len <= 15; ++len) {
        const int c = S::uni((int)cnt[len]);
        left = (left << 1) - c;
        if (left < 0) return false;
        if (c) maxlen = len;
    }
    if (left > 0 && (kind == CNI_KIND_CODES || maxlen > 1)) return false;
    CNI_LANES(l) if (l >= 1 && l < 16) {
        int o = 0;
        for (int k = 1; k < l; ++k) o += cnt[k];
        for (int s = 0; s < n; ++s)
            if (lens[s] == l) symv[o++] = (uint16_t)s;      // o < n: one slot per symbol with a code
    }
    S::sync();
    if (tab) {
        CNI_LANES(l)
            for (int e = l; e < (1 << tab_bits); e += 64) tab[e] = (uint16_t)cni_walk((uint64_t)e, tab_bits, cnt, symv, n);
        S::sync();
    }
    return true;
}

// the literals decoded since the last flush sit in the lanes, byte p in lane p & 63: stored as one wave-wide store
template <class S>
CNI_HD static inline void cni_flush(uint8_t *dst, int32_t &flushed, int32_t out, const uint8_t *lit)
{
    if (flushed == out) return;
    CNI_LANES(l) {
        const int32_t p = flushed + ((l - flushed) & 63);
        if (p < out) dst[p] = lit[S::slot(l)];
    }
    flushed = out;
}

// Raw deflate of src[0 .. n_src) into dst[0 .. n_dst) -> CNI_OK when the stream ended with exactly n_dst bytes, having needed no bit
// behind the input (bytes of the input behind the end of the stream are not looked at, as zlib's inflate() leaves them).
template <class S>
CNI_HD static inline int cni_inflate(const uint8_t *src, int32_t n_src, uint8_t *dst, int32_t n_dst, CniShared &sh)
{
    const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    CniBits b = {src, n_src, 0, 0, 0};
    uint8_t lit[S::SLOTS];
    for (int i = 0; i < S::SLOTS; ++i) lit[i] = 0;
    int32_t out = 0, flushed = 0, fenced = 0;    // bytes decoded / handed to the memory / visible to every lane
    for (int last = 0; !last;) {
        cni_refill(b);
        last = (int)cni_take(b, 1);
        const int type = (int)cni_take(b, 2);
        if (cni_over(b)) return CNI_BAD_INPUT;
        if (type == 3) return CNI_BAD_BLOCK;
        if (type == 0) {
            cni_take(b, b.cnt & 7);
            const int32_t at = b.pos - (b.cnt >> 3);             // the byte the buffer begins with
            if (at < 0 || at > n_src - 4) return CNI_BAD_INPUT;
            const int32_t len = src[at] | (src[at + 1] << 8), nlen = src[at + 2] | (src[at + 3] << 8);
            if ((len ^ 0xFFFF) != nlen) return CNI_BAD_BLOCK;
            if (len > n_src - 4 - at) return CNI_BAD_INPUT;
            if (len > n_dst - out) return CNI_BAD_LENGTH;
            cni_flush<S>(dst, flushed, out, lit);
            CNI_LANES(l)
                for (int32_t i = l; i < len; i += 64) dst[out + i] = src[at + 4 + i];
            out += len;
            flushed = out;
            b.pos = at + 4 + len;
            b.buf = 0;
            b.cnt = 0;
            continue;
        }
        int n_lit = 288, n_dist = 32;
        if (type == 1) {
            CNI_LANES(l) {
                for (int s = l; s < 288; s += 64) sh.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                if (l < 32) sh.lens[288 + l] = 5;
            }
        } else {
            n_lit = 257 + (int)cni_take(b, 5);
            n_dist = 1 + (int)cni_take(b, 5);
            const int n_cl = 4 + (int)cni_take(b, 4);
            if (n_lit > 286 || n_dist > 30) return CNI_BAD_CODES;
            CNI_LANES(l) if (l < 19) sh.cl_lens[l] = 0;
            S::sync();
            for (int i = 0; i < n_cl; ++i) {
                if (b.cnt < 3) cni_refill(b);
                const uint32_t v = cni_take(b, 3);
                if (S::leader()) sh.cl_lens[cl_order[i]] = (uint8_t)v;
            }
            if (cni_over(b)) return CNI_BAD_INPUT;
            if (!cni_build<S>(sh.cl_lens, 19, CNI_KIND_CODES, sh.cl_cnt, sh.cl_sym, nullptr, 0)) return CNI_BAD_CODES;
            int have = 0, prev = 0;
            while (have < n_lit + n_dist) {
                cni_refill(b);
                const int s = cni_symbol<S>(b, nullptr, 0, sh.cl_cnt, sh.cl_sym, 19);
                if (s < 0) return CNI_BAD_CODES;
                int rep = 1, v = s;
                if (s == 16) {
                    if (have == 0) return CNI_BAD_CODES;
                    v = prev;
                    rep = 3 + (int)cni_take(b, 2);
                } else if (s == 17) {
                    v = 0;
                    rep = 3 + (int)cni_take(b, 3);
                } else if (s == 18) {
                    v = 0;
                    rep = 11 + (int)cni_take(b, 7);
                }
                if (cni_over(b)) return CNI_BAD_INPUT;
                if (have + rep > n_lit + n_dist) return CNI_BAD_CODES;
                // the distance lengths go behind the 288 literal/length slots, where the fixed set has them
                CNI_LANES(l)
                    for (int i = l; i < rep; i += 64) {
                        const int at = have + i;
                        sh.lens[at < n_lit ? at : 288 + (at - n_lit)] = (uint8_t)v;
                    }
                have += rep;
                prev = v;
            }
            S::sync();
            if (S::uni((int)sh.lens[256]) == 0) return CNI_BAD_CODES;
        }
        if (!cni_build<S>(sh.lens, n_lit, CNI_KIND_LENS, sh.lit_cnt, sh.lit_sym, sh.lit_tab, CNI_LIT_BITS)) return CNI_BAD_CODES;
        if (!cni_build<S>(sh.lens + 288, n_dist, CNI_KIND_DISTS, sh.dist_cnt, sh.dist_sym, sh.dist_tab, CNI_DIST_BITS)) return CNI_BAD_CODES;
        for (;;) {
            if (b.cnt < 48) cni_refill(b);      // a length (15 + 5) and a distance (15 + 13) take 48 bits; every refill is a load the loop waits for
            int s = cni_symbol<S>(b, sh.lit_tab, CNI_LIT_BITS, sh.lit_cnt, sh.lit_sym, n_lit);
            if (s < 0) return CNI_BAD_SYMBOL;
            if (cni_over(b)) return CNI_BAD_INPUT;
            if (s < 256) {
                if (out >= n_dst) return CNI_BAD_LENGTH;
                S::put(lit, out & 63, (uint8_t)s);
                ++out;
                if (out - flushed == 64) cni_flush<S>(dst, flushed, out, lit);
                continue;
            }
            if (s == 256) break;
            if (s > 285) return CNI_BAD_SYMBOL;
            s -= 257;
            int32_t len = 3 + s;
            if (s == 28) len = 258;
            else if (s >= 8) {
                const int e = (s >> 2) - 1;
                len = ((4 + (s & 3)) << e) + 3 + (int32_t)cni_take(b, e);
            }
            const int ds = cni_symbol<S>(b, sh.dist_tab, CNI_DIST_BITS, sh.dist_cnt, sh.dist_sym, n_dist);
            if (ds < 0 || ds > 29) return CNI_BAD_SYMBOL;
            int32_t dist = 1 + ds;
            if (ds >= 4) {
                const int e = (ds >> 1) - 1;
                dist = ((2 + (ds & 1)) << e) + 1 + (int32_t)cni_take(b, e);
            }
            if (cni_over(b)) return CNI_BAD_INPUT;
            if (dist > out) return CNI_BAD_DISTANCE;
            if (len > n_dst - out) return CNI_BAD_LENGTH;
            cni_flush<S>(dst, flushed, out, lit);
            // the bytes [out - dist, out - dist + min(len, dist)) are read: where other lanes stored some of them since the last fence, fence
            const int32_t span = len < dist ? len : dist;
            if (out - dist + span > fenced) {
                S::sync();
                fenced = out;
            }
            const uint8_t *from = dst + (out - dist);
            if (dist >= len) {
                CNI_LANES(l)
                    for (int32_t i = l; i < len; i += 64) dst[out + i] = from[i];
            } else {
                CNI_LANES(l)
                    for (int32_t i = l; i < len; i += 64) dst[out + i] = from[(uint32_t)i % (uint32_t)dist];
            }
            out += len;
            flushed = out;
        }
    }
    cni_flush<S>(dst, flushed, out, lit);
    if (cni_over(b)) return CNI_BAD_INPUT;
    return out == n_dst ? CNI_OK : CNI_BAD_LENGTH;
}

// ---- CRC-32 (the gzip polynomial, reflected) -----------------------------------------------------------------------------------------
// a(x) b(x) mod P, the coefficient of x^0 in bit 31 (zlib's multmodp())
CNI_HD static inline uint32_t cni_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
CNI_HD static inline uint32_t cni_xpow8(uint32_t n)
{
    uint32_t p = 1u << 31, sq = 1u << 23;
    for (; n; n >>= 1) {
        if (n & 1) p = cni_multmodp(sq, p);
        sq = cni_multmodp(sq, sq);
    }
    return p;
}

// CRC-32 of p[0 .. n): lane l takes the l-th of 64 equal slices, four bytes a step (four tables: the byte-at-a-time chain of table reads is
// what the slice costs), and crc(A B) = crc(A) x^(8 |B|) + crc(B) puts them together.  tab: 4 x 256 words, red: 64 words of shared memory.
// Every lane returns the CRC.
template <class S>
CNI_HD static inline uint32_t cni_crc32(const uint8_t *p, int32_t n, uint32_t *tab, uint32_t *red)
{
    CNI_LANES(l)
        for (int i = l; i < 256; i += 64) {
            uint32_t c = (uint32_t)i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            tab[i] = c;
        }
    S::sync();
    CNI_LANES(l)
        for (int i = l; i < 256; i += 64)
            for (int k = 1; k < 4; ++k) tab[k * 256 + i] = (tab[(k - 1) * 256 + i] >> 8) ^ tab[tab[(k - 1) * 256 + i] & 255];
    S::sync();
    const int32_t slice = (n + 63) / 64;
    CNI_LANES(l) {
        const int32_t a = l * slice < n ? l * slice : n, e = a + slice < n ? a + slice : n;
        uint32_t c = 0xFFFFFFFFu;
        int32_t i = a;
        for (; i + 4 <= e; i += 4) {
            uint32_t w;
            memcpy(&w, p + i, 4);
            c ^= w;
            c = tab[768 + (c & 255)] ^ tab[512 + ((c >> 8) & 255)] ^ tab[256 + ((c >> 16) & 255)] ^ tab[c >> 24];
        }
        for (; i < e; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
        red[l] = e > a ? cni_multmodp(cni_xpow8((uint32_t)(n - e)), ~c) : 0;
    }
    S::sync();
    uint32_t r = 0;
    for (int l = 0; l < 64; ++l) r ^= red[l];
    return r;
}

// ---- the BGZF chain (host) -----------------------------------------------------------------------------------------------------------
struct CniMember {
    int64_t payload;     // offset of the deflate stream from the member's first byte
    int64_t size;        // bytes of the member (BSIZE + 1)
    uint32_t crc, isize;
};
// the member that begins at p, of which `have` bytes are there -> 1: *m is filled and the member lies inside them; 0: more bytes are needed to
// tell; -1: not a BGZF member (gzip magic, deflate, FEXTRA alone among the flags, a `BC` subfield of two bytes, a size that holds header and footer, ISIZE <= 65536)
static inline int cni_bgzf_member(const uint8_t *p, int64_t have, CniMember *m)
{
    static const uint8_t magic[4] = {0x1f, 0x8b, 8, 4};
    for (int i = 0; i < 4 && i < have; ++i)
        if (p[i] != magic[i]) return -1;
    if (have < 12) return 0;
    const int64_t xlen = p[10] | (p[11] << 8);
    if (have < 12 + xlen) return 0;
    int64_t bsize = -1;
    for (int64_t at = 12; at + 4 <= 12 + xlen;) {
        const int64_t slen = p[at + 2] | (p[at + 3] << 8);
        if (at + 4 + slen > 12 + xlen) return -1;
        if (p[at] == 'B' && p[at + 1] == 'C') {
            if (slen != 2) return -1;
            bsize = p[at + 4] | (p[at + 5] << 8);
            break;
        }
        at += 4 + slen;
    }
    if (bsize < 0 || bsize + 1 < 12 + xlen + 8) return -1;
    if (have < bsize + 1) return 0;
    const uint8_t *f = p + bsize + 1 - 8;
    m->payload = 12 + xlen;
    m->size = bsize + 1;
    m->crc = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    m->isize = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
    return m->isize <= 65536 ? 1 : -1;
}

// cornetto_bgzf_scan() (include/cornetto_accel.h)
static inline int cni_bgzf_scan(const uint8_t *buf, int64_t n, int64_t file_off, int64_t *dst, cornetto_bgzf_block_t *blocks, int64_t cap, int64_t *n_blocks,
                                int64_t *resume, int32_t *broken)
{
    int64_t at = 0, k = 0;
    *broken = 0;
    while (at < n && k < cap) {
        CniMember m;
        const int r = cni_bgzf_member(buf + at, n - at, &m);
        if (r < 0) *broken = 1;
        if (r <= 0) break;
        cornetto_bgzf_block_t *b = &blocks[k++];
        b->src = file_off + at + m.payload;
        b->dst = *dst;
        b->n_src = (int32_t)(m.size - m.payload - 8);
        b->n_dst = (int32_t)m.isize;
        b->crc = m.crc;
        b->pad = 0;
        *dst += m.isize;
        at += m.size;
    }
    *n_blocks = k;
    *resume = file_off + at;
    return 0;
}
