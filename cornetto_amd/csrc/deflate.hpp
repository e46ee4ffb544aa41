// deflate.hpp — the BGZF encoder behind cornetto_text_deflate() / cornetto_bamfq_get_bgzf(): ONE source for the device (deflate.hip: a wave
// per BGZF member) and for the CPU (tools/sim/deflate_sim.cc: the same statements with the 64 lanes run one after the other, under the host
// sanitizers against zlib).  A member is made from at most CND_MEMBER bytes:
//   runs      the only matches are byte runs: a run of one value of length >= 4 is its first byte as a literal, then distance-1 matches of
//             258 bytes and one of the remainder (a remainder below 3: literals).  A byte differs from the one in front of it or not: the
//             flags of a tile of 64 bytes are one ballot, the flags of all tiles (1 KiB of them, 8 KiB of LDS) give every byte its run;
//   histogram the literal/length symbols of a tile, equal symbols of the wave put together before the add (DNA text has four hot ones);
//   lengths   the used symbols ranked by (count, symbol) by all lanes, the Huffman depths in place on the sorted counts (Moffat, Katajainen)
//             by one lane, lengths above the limit folded to it and the Kraft sum mended from the longest codes upwards;
//   header    a dynamic block whose code lengths are sent one by one (no repeat codes), the distance set has one code of one bit or none;
//   stream    a tile's codes go to the bit offsets a wave prefix sum of their sizes gives, ORed into 64 zeroed words of LDS, whose whole words
//             leave with one wave-wide store: no byte of the result depends on the order of the lanes;
//   stored    a block that would not be smaller than the bytes themselves is stored: a member is at most CND_MEMBER + 5 + 26 bytes.
// The lane shim S is that of inflate.hpp (first, step, slot, leader, sync, uni) and, because lanes speak to each other here:
//   S::ballot(f)      bit l: f of lane l            S::scan(v, ex)   ex of lane l = v of the lanes in front of it; -> the sum
//   S::pick(v, lane)  v of that lane                S::lds_or / S::lds_add    an atomic of shared memory (plain on the CPU)
// Bounds come from the code, never from the data: n is cut to CND_MEMBER, every symbol index is below CND_SYMS by construction and
// checked, a tile puts at most 64 codes of at most 21 bits into 64 words, and the dynamic block is written only when its size, known from
// the histogram beforehand, is below the stored one: inside [out, out + CND_STRIDE).
#pragma once
#include "inflate.hpp"

enum {
    CND_MEMBER = 0xff00,     // payload bytes of a member at most (what bgzip uses)
    CND_STRIDE = 65536,      // bytes of staging per member; the member itself is [CND_HEAD, CND_HEAD + size)
    CND_HEAD = 14,           // ... so that the deflate stream begins at a multiple of four
    CND_PAYLOAD = 32,
    CND_MAX_SIZE = CND_MEMBER + 5 + 26,
    CND_TILES = 1024,
    CND_SYMS = 288,
    CND_NONE = 0xFFFF
};

// per wave, in LDS on the device: 14.5 KiB
struct CndShared {
    union {
        struct {
            uint32_t tab[4 * 256], red[64];
        } crc;                                   // first the CRC-32 of the bytes,
        struct {
            uint64_t mask[CND_TILES];            // then the run flags of every tile
            uint16_t nxt[CND_TILES];             // ... and the first flag behind the tile
        } run;
    } u;
    uint32_t freq[CND_SYMS], work[CND_SYMS];
    uint16_t order[CND_SYMS], code[CND_SYMS];
    uint8_t len[CND_SYMS];
    uint32_t cl_freq[20];
    uint16_t cl_code[20];
    uint8_t cl_len[20];
    uint32_t cnt[16], red[64], buf[64];
    uint16_t blk[64];
};

CNI_HD static inline int cnd_clz64(uint64_t v) { return __builtin_clzll(v); }
CNI_HD static inline int cnd_ctz64(uint64_t v) { return __builtin_ctzll(v); }

// byte l of tile t lies in the run [s, e): m the tile's flags, prv the last flag in front of the tile, nxt the first one behind it
CNI_HD static inline void cnd_run(uint64_t m, int l, int32_t t, int32_t prv, int32_t nxt, int32_t &s, int32_t &e)
{
    const uint64_t low = m & (~0ull >> (63 - l));
    s = low ? t * 64 + 63 - cnd_clz64(low) : prv;
    const uint64_t high = l < 63 ? m >> (l + 1) : 0;
    e = high ? t * 64 + l + 1 + cnd_ctz64(high) : nxt;
}

// what byte p of the run [s, e) is in the stream -> 0: nothing (inside a match), 1: a literal, else the length of the match that begins here
CNI_HD static inline int cnd_token(int32_t p, int32_t s, int32_t e)
{
    const int32_t len = e - s, k = p - s;
    if (len < 4 || k <= 0) return 1;
    const int32_t j = k - 1, chunk = j / 258, within = j - chunk * 258;
    int32_t cl = (len - 1) - chunk * 258;
    if (cl > 258) cl = 258;
    if (cl < 3) return 1;
    return within == 0 ? cl : 0;
}

// the length symbol of a match of 3 .. 258 bytes, its extra bits and their value
CNI_HD static inline void cnd_lensym(int len, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    const uint32_t x = (uint32_t)(len - 3);
    eb = ev = 0;
    if (len >= 258) sym = 285;
    else if (x < 8) sym = 257 + x;
    else {
        const uint32_t e = (uint32_t)(29 - __builtin_clz(x));      // x in [4 << e, 8 << e)
        sym = 257 + 4 * e + (x >> e);
        eb = e;
        ev = x & ((1u << e) - 1);
    }
}
CNI_HD static inline uint32_t cnd_extra_bits(int sym)
{
    const int s = sym - 257;
    return s < 8 || s >= 28 ? 0u : (uint32_t)((s >> 2) - 1);
}

// the symbol of position p (CND_NONE: none) and, for the stream, its extra bits
template <class S>
CNI_HD static inline uint32_t cnd_symbol(const uint8_t *src, int32_t n, uint64_t m, int l, int32_t t, int32_t prv, int32_t nxt, uint32_t &eb, uint32_t &ev)
{
    const int32_t p = t * 64 + l;
    eb = ev = 0;
    if (p > n) return CND_NONE;
    if (p == n) return 256;
    int32_t s, e;
    cnd_run(m, l, t, prv, nxt, s, e);
    const int k = cnd_token(p, s, e);
    if (k == 0) return CND_NONE;
    if (k == 1) return src[p];
    uint32_t sym;
    cnd_lensym(k, sym, eb, ev);
    return sym;
}

// A complete prefix code of at most `limit` bits for the symbols with a count: len[0 .. n).  One symbol alone gets one bit, and so does a
// second one nobody sends (a code set every decoder takes).
template <class S>
CNI_HD static inline void cnd_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, CndShared &sh)
{
    S::sync();
    CNI_LANES(l) {
        uint32_t used = 0;
        for (int s = l; s < n; s += 64) {
            len[s] = 0;
            const uint32_t f = freq[s];
            if (!f) continue;
            ++used;
            int r = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t g = freq[j];
                r += (g && (g < f || (g == f && j < s))) ? 1 : 0;
            }
            sh.order[r] = (uint16_t)s;                   // r < the number of used symbols <= n
            sh.work[r] = f;
        }
        sh.red[l] = used;
    }
    S::sync();
    int m = 0;
    for (int l = 0; l < 64; ++l) m += (int)sh.red[l];
    m = S::uni(m);
    if (S::leader() && m == 1) {
        len[sh.order[0]] = 1;
        len[sh.order[0] == 0 ? 1 : 0] = 1;
    }
    if (S::leader() && m >= 2) {
        uint32_t *A = sh.work;
        // the depths of the leaves of the Huffman tree, in place on the ascending counts
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < m - 1; ++next) {
            if (leaf >= m || A[root] < A[leaf]) {
                A[next] = A[root];
                A[root++] = (uint32_t)next;
            } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) {
                A[next] += A[root];
                A[root++] = (uint32_t)next;
            } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (int next = m - 3; next >= 0; --next) A[next] = A[A[next] < (uint32_t)m ? A[next] : 0] + 1;
        int avbl = 1, used = 0, dpth = 0, next = m - 1;
        root = m - 2;
        while (avbl > 0 && next >= 0) {
            while (root >= 0 && (int)A[root] == dpth) {
                ++used;
                --root;
            }
            while (avbl > used && next >= 0) {
                A[next--] = (uint32_t)dpth;
                --avbl;
            }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
        // the limit: longer codes become `limit` bits, and as long as the set is over-subscribed a code of `limit` bits and the longest
        // shorter code become two codes one bit below the latter (the Kraft sum falls by one unit of 2^-limit a turn, n units at most)
        for (int d = 0; d < 16; ++d) sh.cnt[d] = 0;
        for (int i = 0; i < m; ++i) {
            const int d = (int)A[i] > limit ? limit : (int)A[i] < 1 ? 1 : (int)A[i];
            sh.cnt[d] += 1;
        }
        uint32_t total = 0;
        for (int d = 1; d <= limit; ++d) total += sh.cnt[d] << (limit - d);
        for (int g = 0; g < n && total > (1u << limit) && sh.cnt[limit] > 0; ++g) {
            sh.cnt[limit] -= 1;
            for (int d = limit - 1; d >= 1; --d)
                if (sh.cnt[d]) {
                    sh.cnt[d] -= 1;
                    sh.cnt[d + 1] += 2;
                    break;
                }
            total -= 1;
        }
        int i = 0;
        for (int d = limit; d >= 1; --d)
            for (uint32_t k = 0; k < sh.cnt[d] && i < m; ++k) len[sh.order[i++]] = (uint8_t)d;      // the rarest symbols take the longest codes
    }
    S::sync();
}

// the canonical codes of len[0 .. n), bit-reversed: ready for a stream that is filled from its low bits
template <class S>
CNI_HD static inline void cnd_codes(const uint8_t *len, int n, uint16_t *code, CndShared &sh)
{
    S::sync();
    CNI_LANES(l) if (l < 16) {
        uint32_t c = 0;
        for (int s = 0; s < n; ++s) c += len[s] == l;
        sh.cnt[l] = l ? c : 0;
    }
    S::sync();
    CNI_LANES(l)
        for (int s = l; s < n; s += 64) {
            const int L = len[s] & 15;
            uint32_t c = 0;
            for (int b = 1; b <= L; ++b) c = (c + sh.cnt[b - 1]) << 1;
            for (int j = 0; j < s; ++j) c += len[j] == L;
            uint32_t r = 0;
            for (int b = 0; b < L; ++b) r |= ((c >> b) & 1u) << (L - 1 - b);
            code[s] = (uint16_t)r;
        }
    S::sync();
}

// The codes of a tile — lane l: the low nb (<= 32) bits of `bits` — behind bit `bitpos` of the stream outw[0 .. out_words): ORed into the
// tile's 64 words (sh.buf; word 0 holds the open word of the stream, the others are zero), whose whole words are stored.
template <class S>
CNI_HD static inline void cnd_put(const uint32_t *bits, const uint32_t *nb, uint32_t &bitpos, uint32_t *outw, uint32_t out_words, CndShared &sh)
{
    uint32_t ex[S::SLOTS];
    const uint32_t total = S::uni(S::scan(nb, ex)), base = bitpos & 31;
    CNI_LANES(l) {
        const uint32_t k = nb[S::slot(l)];
        if (k) {
            const uint32_t o = base + ex[S::slot(l)], w = o >> 5;
            const uint64_t v = (uint64_t)(bits[S::slot(l)] & (k >= 32 ? ~0u : (1u << k) - 1)) << (o & 31);
            if (w < 63) {
                S::lds_or(&sh.buf[w], (uint32_t)v);
                if (v >> 32) S::lds_or(&sh.buf[w + 1], (uint32_t)(v >> 32));
            }
        }
    }
    S::sync();
    const uint32_t nw = (base + total) >> 5, w0 = bitpos >> 5;
    CNI_LANES(l) if ((uint32_t)l < nw && w0 + (uint32_t)l < out_words) outw[w0 + (uint32_t)l] = sh.buf[l];
    const uint32_t open = nw < 64 ? sh.buf[nw] : 0;
    S::sync();
    CNI_LANES(l) sh.buf[l] = l == 0 ? open : 0;
    S::sync();
    bitpos += total;
}

// The BGZF member of src[0 .. n), n <= CND_MEMBER (more is cut): its bytes are out[CND_HEAD .. CND_HEAD + size), out a multiple of four with
// CND_STRIDE bytes -> size.  Every lane returns it.
template <class S>
CNI_HD static inline int32_t cnd_member(const uint8_t *src, int32_t n, uint8_t *out, CndShared &sh)
{
    const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (n < 0) n = 0;
    if (n > CND_MEMBER) n = CND_MEMBER;
    const uint32_t crc = cni_crc32<S>(src, n, sh.u.crc.tab, sh.u.crc.red);
    S::sync();
    const int32_t tiles = (n + 64) >> 6;                  // of the positions 0 .. n: position n is the end of the block
    // ---- the runs: a flag where a byte differs from the one in front of it, and at 0 and n
    for (int32_t t = 0; t < tiles; ++t) {
        bool f[S::SLOTS];
        CNI_LANES(l) {
            const int32_t p = t * 64 + l;
            f[S::slot(l)] = p <= n && (p == 0 || p == n || src[p] != src[p - 1]);
        }
        const uint64_t m = S::ballot(f);
        if (S::leader()) sh.u.run.mask[t] = m;
    }
    S::sync();
    // the first flag behind every tile: a lane takes 16 tiles from the last to the first, then what the lanes behind it found (a flag stands at n)
    CNI_LANES(l) {
        uint32_t first = CND_NONE;
        for (int32_t t = l * 16 + 15; t >= l * 16; --t) {
            if (t >= tiles) continue;
            sh.u.run.nxt[t] = (uint16_t)first;
            const uint64_t m = sh.u.run.mask[t];
            if (m) first = (uint32_t)(t * 64 + cnd_ctz64(m));
        }
        sh.blk[l] = (uint16_t)first;
    }
    S::sync();
    CNI_LANES(l) {
        uint32_t first = CND_NONE;
        for (int k = l + 1; k < 64 && first == CND_NONE; ++k) first = sh.blk[k];
        if (first == CND_NONE) first = (uint32_t)n;
        for (int32_t t = l * 16; t < l * 16 + 16 && t < tiles; ++t)
            if (sh.u.run.nxt[t] == CND_NONE) sh.u.run.nxt[t] = (uint16_t)first;
    }
    CNI_LANES(l)
        for (int s = l; s < CND_SYMS; s += 64) sh.freq[s] = 0;
    S::sync();
    // ---- the histogram of the literal/length symbols
    int32_t prv = 0;
    for (int32_t t = 0; t < tiles; ++t) {
        const uint64_t m = sh.u.run.mask[t];
        const int32_t nxt = sh.u.run.nxt[t];
        uint32_t sym[S::SLOTS];
        bool act[S::SLOTS], eq[S::SLOTS];
        CNI_LANES(l) {
            uint32_t eb, ev;
            sym[S::slot(l)] = cnd_symbol<S>(src, n, m, l, t, prv, nxt, eb, ev);
            act[S::slot(l)] = sym[S::slot(l)] < CND_SYMS;
        }
        for (int round = 0; round < 8; ++round) {        // equal symbols of the wave are one add
            const uint64_t live = S::ballot(act);
            if (!live) break;
            const uint32_t v = S::uni(S::pick(sym, cnd_ctz64(live)));
            CNI_LANES(l) eq[S::slot(l)] = act[S::slot(l)] && sym[S::slot(l)] == v;
            const uint64_t grp = S::ballot(eq);
            if (S::leader() && v < CND_SYMS) S::lds_add(&sh.freq[v], (uint32_t)__builtin_popcountll(grp));
            CNI_LANES(l) if (eq[S::slot(l)]) act[S::slot(l)] = false;
        }
        CNI_LANES(l) if (act[S::slot(l)]) S::lds_add(&sh.freq[sym[S::slot(l)]], 1u);
        if (m) prv = t * 64 + 63 - cnd_clz64(m);
    }
    // ---- the two code sets
    cnd_lengths<S>(sh.freq, 286, 15, sh.len, sh);
    int n_lit = 286;
    while (n_lit > 257 && S::uni((int)sh.len[n_lit - 1]) == 0) --n_lit;
    const int dist_len = n_lit > 257 ? 1 : 0;            // the one distance code, if there is a match
    CNI_LANES(l) if (l < 20) {
        uint32_t c = 0;
        if (l < 16) {
            for (int s = 0; s < n_lit; ++s) c += sh.len[s] == l;
            c += dist_len == l;
        }
        sh.cl_freq[l] = c;
    }
    cnd_lengths<S>(sh.cl_freq, 19, 7, sh.cl_len, sh);
    cnd_codes<S>(sh.len, 286, sh.code, sh);
    cnd_codes<S>(sh.cl_len, 19, sh.cl_code, sh);
    // ---- the size of the dynamic block, from the counts
    CNI_LANES(l) {
        uint32_t b = 0;
        for (int s = l; s < 286; s += 64) b += sh.freq[s] * ((uint32_t)sh.len[s] + (s > 256 ? cnd_extra_bits(s) + 1u : 0u));
        if (l < 16) b += sh.cl_freq[l] * sh.cl_len[l];
        sh.red[l] = b;
    }
    S::sync();
    uint32_t dyn_bits = 3 + 14 + 19 * 3;
    for (int l = 0; l < 64; ++l) dyn_bits += sh.red[l];
    dyn_bits = S::uni(dyn_bits);
    const int32_t dyn_bytes = (int32_t)((dyn_bits + 7) >> 3);
    int32_t pay;
    if (dyn_bytes >= n + 5) {
        // ---- stored
        pay = n + 5;
        CNI_LANES(l) if (l < 5) out[CND_PAYLOAD + l] = (uint8_t)(l == 0 ? 1 : l == 1 ? n : l == 2 ? n >> 8 : l == 3 ? ~n : ~n >> 8);
        CNI_LANES(l)
            for (int32_t i = l; i < n; i += 64) out[CND_PAYLOAD + 5 + i] = src[i];
    } else {
        pay = dyn_bytes;
        uint32_t *outw = reinterpret_cast<uint32_t *>(out + CND_PAYLOAD);
        const uint32_t out_words = (CND_STRIDE - CND_PAYLOAD - 8) / 4;
        uint32_t bitpos = 0;
        uint32_t bits[S::SLOTS], nb[S::SLOTS];
        CNI_LANES(l) sh.buf[l] = 0;
        S::sync();
        // the block header and the 19 lengths of the code-length code: a field per lane
        CNI_LANES(l) {
            uint32_t v = 0, k = 0;
            if (l == 0) { v = 1 | (2 << 1); k = 3; }
            else if (l == 1) { v = (uint32_t)(n_lit - 257); k = 5; }
            else if (l == 2) { v = 0; k = 5; }
            else if (l == 3) { v = 15; k = 4; }
            else if (l < 23) { v = sh.cl_len[cl_order[l - 4]]; k = 3; }
            bits[S::slot(l)] = v;
            nb[S::slot(l)] = k;
        }
        cnd_put<S>(bits, nb, bitpos, outw, out_words, sh);
        // the code lengths, one code each
        for (int i0 = 0; i0 < n_lit + 1; i0 += 64) {
            CNI_LANES(l) {
                const int i = i0 + l;
                const int v = i < n_lit ? sh.len[i] : dist_len;
                bits[S::slot(l)] = i <= n_lit ? sh.cl_code[v & 15] : 0;
                nb[S::slot(l)] = i <= n_lit ? sh.cl_len[v & 15] : 0;
            }
            cnd_put<S>(bits, nb, bitpos, outw, out_words, sh);
        }
        // the symbols
        prv = 0;
        for (int32_t t = 0; t < tiles; ++t) {
            const uint64_t m = sh.u.run.mask[t];
            const int32_t nxt = sh.u.run.nxt[t];
            CNI_LANES(l) {
                uint32_t eb, ev;
                const uint32_t s = cnd_symbol<S>(src, n, m, l, t, prv, nxt, eb, ev);
                uint32_t v = 0, k = 0;
                if (s < CND_SYMS) {
                    v = sh.code[s];
                    k = sh.len[s];
                    if (s > 256) {                       // extra bits of the length, then the distance code: 0, one bit
                        v |= ev << k;
                        k += eb + 1;
                    }
                }
                bits[S::slot(l)] = v;
                nb[S::slot(l)] = k;
            }
            cnd_put<S>(bits, nb, bitpos, outw, out_words, sh);
            if (m) prv = t * 64 + 63 - cnd_clz64(m);
        }
        if (S::leader() && (bitpos & 31) && (bitpos >> 5) < out_words) outw[bitpos >> 5] = sh.buf[0];
        pay = (int32_t)((bitpos + 7) >> 3);
    }
    S::sync();
    const int32_t size = 18 + pay + 8;
    CNI_LANES(l) {
        const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(size - 1), (uint8_t)((size - 1) >> 8)};
        if (l < 18) out[CND_HEAD + l] = head[l];
        if (l < 4) out[CND_PAYLOAD + pay + l] = (uint8_t)(crc >> (8 * l));
        else if (l < 8) out[CND_PAYLOAD + pay + l] = (uint8_t)((uint32_t)n >> (8 * (l - 4)));
    }
    S::sync();
    return size;
}
