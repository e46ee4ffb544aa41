// fqrec.hpp — the plain four-line FASTQ record on the device, shared by fastq.hip (cornetto_fastq_split: the records in front of sdust /
// telofind) and fqseq.hip (cornetto_fqseq_*: the text `seq` prints): the newline mask the index of marks.hpp is built from, and fq_records,
// the checks under which kseq_read (src/kseq.h:184-224) reads exactly four lines as one record.  One statement of the rules for both.
// tools/sim/fqseq_sim.cc compiles fq_frame() for the CPU (tests/test_fqseq_host.py runs it under the host sanitizers).
#pragma once
#include <cstdint>

#include "../../include/cornetto_accel.h"

#ifdef __HIPCC__
#include "common.hpp"
#define FQ_HD __host__ __device__
#else
#define FQ_HD
#endif

namespace {   // internal linkage: every translation unit that includes this gets its own copy

#ifdef __HIPCC__
// bit i = byte i of the 16-byte piece at `pos` has the value C
template <uint8_t C>
__device__ __forceinline__ uint32_t byte_mask16(const uint8_t *text, int64_t pos, int64_t n)
{
    uint32_t m = 0;
    if (pos + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = w[k] ^ (0x01010101u * C);                  // zero byte <=> the value
            const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every zero byte (exact)
            m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) m |= (uint32_t)(pos + i < n && text[pos + i] == C) << i;
    }
    return m;
}

// bit i = byte i of the 16-byte piece at `pos` is '\n'
__device__ __forceinline__ uint32_t nl_mask16(const uint8_t *text, int64_t pos, int64_t n) { return byte_mask16<'\n'>(text, pos, n); }
#endif

FQ_HD static inline bool fq_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace(), C locale

// Line k of the piece is [k == 0 ? 0 : nl[k-1] + 1, nl[k]); with `virt` the text ends inside its last line and that line's
// end is n itself (kseq treats the end of the input as the end of the line, src/kseq.h:127-131).
struct FqArgs {
    const uint8_t *text;
    int64_t n;
    const uint32_t *nl;
    int64_t n_nl;      // real newlines
    int64_t n_rec;     // groups of four lines to look at
    int32_t min_len;
    cornetto_fqrec_t *recs;
    uint32_t *first_bad;   // smallest group that is not a plain record
    uint32_t *ends;        // [n_rec] offset just behind the group
};

// group r of four lines -> its record and the offset just behind it; false: not a plain record
FQ_HD static inline bool fq_frame(const FqArgs &A, int64_t r, cornetto_fqrec_t &rec, uint32_t &end)
{
    const uint8_t *t = A.text;
    int64_t e[4];
    for (int k = 0; k < 4; ++k) e[k] = 4 * r + k < A.n_nl ? (int64_t)A.nl[4 * r + k] : A.n;
    const int64_t s0 = r == 0 ? 0 : (int64_t)A.nl[4 * r - 1] + 1, s1 = e[0] + 1, s2 = e[1] + 1, s3 = e[2] + 1;
    bool ok = t[s0] == '@';                                            // kseq_read :189-193 takes the next '@' or '>' anywhere: it must be right here
    // :201-205 the sequence ends at a line that begins with '>', '+' or '@'; an empty line is skipped
    if (e[1] > s1) ok = ok && t[s1] != '>' && t[s1] != '+' && t[s1] != '@';
    ok = ok && e[2] > s2 && t[s2] == '+';                              // one sequence line only, then the separator
    int64_t l1 = e[1] - s1, l3 = e[3] - s3;
    if (l1 > 1 && t[e[1] - 1] == '\r') --l1;                           // :138, for the sequence as a whole
    if (l3 > 1 && t[e[3] - 1] == '\r') --l3;
    ok = ok && l1 == l3 && l1 <= 0x7fffffffLL;                         // :221-223: the first quality line must complete the record
    // name / comment, :195-196
    int64_t j = s0 + 1;
    while (j < e[0] && !fq_space(t[j])) ++j;
    int64_t cl = j < e[0] ? e[0] - (j + 1) : 0;
    if (cl > 1 && t[e[0] - 1] == '\r') --cl;
    ok = ok && (j - (s0 + 1)) <= 0x7fffffffLL && cl <= 0x7fffffffLL;
    rec.head = s0;
    rec.seq = s1;
    rec.qual = s3;
    rec.len = (int32_t)l1;
    rec.name_len = (int32_t)(j - (s0 + 1));
    rec.comment_len = (int32_t)cl;
    rec.keep = l1 >= A.min_len ? 1 : 0;
    end = (uint32_t)(e[3] < A.n ? e[3] + 1 : A.n);
    return ok;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(256) void fq_records(FqArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rec) return;
    cornetto_fqrec_t rec;
    uint32_t end;
    const bool ok = fq_frame(A, r, rec, end);
    A.recs[r] = rec;
    A.ends[r] = end;
    if (!ok) atomicMin(A.first_bad, (uint32_t)r);
}
#endif

}  // namespace
