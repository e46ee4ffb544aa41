// qmean.hpp — the segmented sum of quality weights behind `seq -q` (include/cornetto_accel.h states the rule), shared by fqseq.hip and
// bamfq.hip through qmean.hip.  The input is a window of bytes and a table of ranges start[r] (ascending), len[r] that do not overlap; a
// range of length 0 costs nothing (a record that the length or duplex filter dropped).  The decomposition of qmean_sum:
//   a wave owns QM_CHUNK = 1 KiB of the window, a lane one aligned 16-byte piece of it;
//   qm_first()   the first range that reaches into the chunk: a binary search over the ranges' ends, the same in every lane.  A chunk of
//                names and bases leaves here without a load of text;
//   qm_span()    per range that meets the chunk, the bytes [lo, hi) of the lane's piece that belong to it;
//   qm_lane()    their weights out of a 256-entry table (the clamps folded in: qm_weight()), added in 64 bits;
//   then a wave reduction and ONE 64-bit atomic add to sum[r] by one lane: a 30 kb read costs about 30 atomics.
// Host/device functions, so that tools/sim/qmean_sim.cc runs the same index arithmetic on the CPU under the host sanitizers
// (tests/test_qmean_host.py).  Nothing here reads outside text[0, n_text rounded up to 16), start[0, n), len[0, n) and tab[0, 256).
#pragma once
#include <cstdint>

#include "../../include/cornetto_accel.h"

#ifdef __HIPCC__
#define QM_HD __host__ __device__
#else
#define QM_HD
#endif

namespace {   // internal linkage: every translation unit that includes this gets its own copy

constexpr int QM_LANES = 64;
constexpr int QM_CHUNK = QM_LANES * 16;       // bytes of the window per wave
constexpr int QM_WAVES = 4;                   // waves per workgroup

// E[clamp(q, 0, 93)]
QM_HD static inline uint32_t qm_e(int q)
{
    constexpr uint32_t E[CORNETTO_QUAL_MAX + 1] = CORNETTO_QUAL_WEIGHTS;
    return E[q < 0 ? 0 : q > CORNETTO_QUAL_MAX ? CORNETTO_QUAL_MAX : q];
}

// entry `byte` of the 256-entry table: a printed FASTQ character (bam == 0: q = byte - 33) or a raw BAM quality (q = byte), clamped
QM_HD static inline uint32_t qm_weight(int byte, int bam) { return qm_e(bam ? byte : byte - 33); }

// the first range r with start[r] + len[r] > c0, or n (the ends do not descend: ranges are ascending and do not overlap)
QM_HD static inline int64_t qm_first(const uint32_t *start, const uint32_t *len, int64_t n, int64_t c0)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)start[mid] + (int64_t)len[mid] > c0) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the bytes [lo, hi) of the 16-byte piece at `pos` that lie in the range [s, e); lo >= hi: none
QM_HD static inline void qm_span(int64_t pos, int64_t s, int64_t e, int &lo, int &hi)
{
    const int64_t a = s - pos, b = e - pos;
    lo = a < 0 ? 0 : a > 16 ? 16 : (int)a;
    hi = b < 0 ? 0 : b > 16 ? 16 : (int)b;
}

// the weights of bytes [lo, hi) of the piece w[0 .. 4) (little endian)
QM_HD static inline uint64_t qm_lane(const uint32_t w[4], int lo, int hi, const uint32_t *tab)
{
    uint64_t acc = 0;
    for (int j = 0; j < 16; ++j) {      // (a constant trip count: unrolled, every shift a constant)
        const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const uint32_t v = tab[c];
        acc += (j >= lo && j < hi) ? v : 0u;
    }
    return acc;
}

}  // namespace
