// fqseq.hpp — what one thread of fqseq_text (fqseq.hip) does for its 16 output bytes, and the size of a record's text: host/device functions, so
// that tools/sim/fqseq_sim.cc runs the same index arithmetic on the CPU under the host sanitizers (tests/test_fqseq_host.py).
#pragma once
#include <cstdint>
#include <cstring>

#include "fqrec.hpp"

namespace {   // internal linkage: every translation unit that includes this gets its own copy

struct Fx16 {
    uint32_t w[4];
};

// bytes of the record's text: 0 for a record that -m drops
FQ_HD static inline uint32_t fx_size(const cornetto_fqrec_t &x)
{
    if (!x.keep) return 0u;
    return 1u + (uint32_t)x.name_len + (x.comment_len ? 1u + (uint32_t)x.comment_len : 0u) + 1u + (uint32_t)x.len + 1u + 2u + (uint32_t)x.len + 1u;
}

struct FxArgs {
    const uint8_t *text;             // the window (readable 256 bytes beyond its end)
    const cornetto_fqrec_t *recs;    // offsets into the window
    const uint32_t *out;             // [n + 1]
    int64_t n, at, nbytes;
    uint8_t *dst;                    // at least nbytes rounded up to 16
};

// largest r in [lo, hi] with out[r] <= p (records without text share their offset with the next one: the one found has text when p < out[n])
FQ_HD static inline int64_t fx_find(const uint32_t *out, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)out[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// byte k of the record's text, k < its size
FQ_HD static inline uint8_t fx_byte(const uint8_t *t, const cornetto_fqrec_t &r, int64_t k)
{
    if (k == 0) return '@';
    k -= 1;
    if (k < r.name_len) return t[r.head + 1 + k];
    k -= r.name_len;
    if (r.comment_len) {
        if (k == 0) return '\t';       // in place of whatever white-space byte stood there
        k -= 1;
        if (k < r.comment_len) return t[r.head + r.name_len + 2 + k];
        k -= r.comment_len;
    }
    if (k == 0) return '\n';
    k -= 1;
    if (k < r.len) return t[r.seq + k];
    k -= r.len;
    if (k < 3) return k == 1 ? '+' : '\n';
    k -= 3;
    if (k < r.len) return t[r.qual + k];
    return '\n';
}

// where the 16 bytes of the record's text from byte k0 on stand in the window when they are 16 consecutive bytes of one payload; -1 otherwise
FQ_HD static inline int64_t fx_run16(const cornetto_fqrec_t &r, int64_t k0)
{
    const int64_t nl = r.name_len, cl = r.comment_len, len = r.len;
    if (k0 >= 1 && k0 + 16 <= 1 + nl) return r.head + k0;
    const int64_t c0 = k0 - (2 + nl);
    if (cl && c0 >= 0 && c0 + 16 <= cl) return r.head + nl + 2 + c0;
    const int64_t h = 1 + nl + (cl ? 1 + cl : 0) + 1;
    const int64_t b0 = k0 - h;
    if (b0 >= 0 && b0 + 16 <= len) return r.seq + b0;
    const int64_t q0 = b0 - (len + 3);
    if (q0 >= 0 && q0 + 16 <= len) return r.qual + q0;
    return -1;
}

// 16 bytes from any address: the two aligned 16-byte pieces that hold them, shifted into place (the window is readable beyond its end)
FQ_HD static inline Fx16 fx_load16(const uint8_t *text, int64_t src)
{
    const int64_t a = src & ~(int64_t)15;
    const int sh = (int)(src & 15), d = sh >> 2, b = 8 * (sh & 3);
    uint32_t w[8];
#ifdef __HIP_DEVICE_COMPILE__
    const uint4 A = *reinterpret_cast<const uint4 *>(text + a);
    const uint4 B = *reinterpret_cast<const uint4 *>(text + a + 16);
    w[0] = A.x; w[1] = A.y; w[2] = A.z; w[3] = A.w;
    w[4] = B.x; w[5] = B.y; w[6] = B.z; w[7] = B.w;
#else
    memcpy(w, text + a, 32);
#endif
    uint32_t x[5];
    for (int k = 0; k < 5; ++k) x[k] = d == 0 ? w[k] : d == 1 ? w[k + 1] : d == 2 ? w[k + 2] : w[k + 3];
    uint32_t o[4];
    for (int k = 0; k < 4; ++k) o[k] = (uint32_t)((((uint64_t)x[k + 1] << 32) | x[k]) >> b);
    return Fx16{{o[0], o[1], o[2], o[3]}};
}

// The bytes [p, p + m) of the text that begins at A.at, m in 1 .. 16 and p + m <= out[n], as the low m bytes of the result (little endian); the rest is 0.
// [r0, r1]: records that hold every byte of the range (a tile's, found once).
FQ_HD static inline Fx16 fx_chunk(const FxArgs &A, int64_t r0, int64_t r1, int64_t p, int m)
{
    int64_t ri = fx_find(A.out, r0, r1, p);
    cornetto_fqrec_t r = A.recs[ri];
    int64_t o = A.out[ri];
    const int64_t src = m == 16 ? fx_run16(r, p - o) : -1;
    if (src >= 0) return fx_load16(A.text, src);
    int64_t o1 = A.out[ri + 1];
    uint64_t v0 = 0, v1 = 0;
    for (int j = 0; j < m; ++j) {
        const int64_t q = p + j;
        if (q >= o1) {                      // (q < out[n]: there is a record with text behind this one, inside [ri + 1, r1])
            ri = fx_find(A.out, ri + 1, r1, q);
            r = A.recs[ri];
            o = A.out[ri];
            o1 = A.out[ri + 1];
        }
        const uint64_t c = (uint64_t)fx_byte(A.text, r, q - o) << (8 * (j & 7));
        if (j < 8) v0 |= c;
        else v1 |= c;
    }
    return Fx16{{(uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32)}};
}

}  // namespace
