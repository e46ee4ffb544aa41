// qmean.hip — qmean_sum: the sums of quality weights of `seq -q` over a window and its table of ranges (qmean.hpp has the decomposition and
// the arithmetic; include/cornetto_accel.h the rule).  One kernel for the FASTQ window of fqseq.hip (printed characters) and the inflated
// BAM window of bamfq.hip (raw qualities): the two differ in the 256-entry weight table the workgroup builds in LDS.  The caller zeroes
// sum[] for every window and passes a window that is readable to the next multiple of 16 (both windows have 256 bytes behind them).
#include "common.hpp"
#include "internal.hpp"
#include "qmean.hpp"

namespace {

__device__ __forceinline__ unsigned long long qm_wave_sum(unsigned long long s)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__global__ void __launch_bounds__(QM_WAVES *QM_LANES) qmean_sum(const uint8_t *__restrict__ text, int64_t n_text, const uint32_t *__restrict__ start,
                                                                 const uint32_t *__restrict__ len, int64_t n, int bam, unsigned long long *__restrict__ sum)
{
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = qm_weight((int)threadIdx.x, bam);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int64_t c0 = ((int64_t)blockIdx.x * QM_WAVES + wave) * QM_CHUNK;
    if (c0 >= n_text) return;
    const int64_t c1 = n_text - c0 < QM_CHUNK ? n_text : c0 + QM_CHUNK;
    int64_t r = qm_first(start, len, n, c0);                  // (uniform: scalar loads)
    if (r >= n || (int64_t)start[r] >= c1) return;
    const int64_t pos = c0 + (int64_t)lane * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (pos < c1) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    for (; r < n; ++r) {
        const int64_t s = (int64_t)start[r];
        if (s >= c1) break;
        const int64_t e = s + (int64_t)len[r];
        if (e <= s || e <= c0) continue;
        int lo, hi;
        qm_span(pos, s, e < c1 ? e : c1, lo, hi);
        const unsigned long long acc = qm_wave_sum((unsigned long long)qm_lane(w, lo, hi, tab));
        if (lane == 0) atomicAdd(sum + r, acc);
    }
}

}  // namespace

int cn_qmean_sum(cornetto_accel_t *h, const uint8_t *d_text, int64_t n_text, const uint32_t *d_start, const uint32_t *d_len, int64_t n, int bam, unsigned long long *d_sum)
{
    if (n <= 0 || n_text <= 0) return CORNETTO_OK;
    const int64_t blocks = (n_text + (int64_t)QM_WAVES * QM_CHUNK - 1) / ((int64_t)QM_WAVES * QM_CHUNK);
    if (blocks > INT32_MAX) return cn_fail(h, CORNETTO_E_ARG, "qmean_sum: a window of %lld bytes is too large", (long long)n_text);
    CN_LAUNCH(h, "qmean_sum", qmean_sum<<<dim3((unsigned)blocks), dim3(QM_WAVES * QM_LANES), 0, h->stream>>>(d_text, n_text, d_start, d_len, n, bam, d_sum));
    return CORNETTO_OK;
}

extern "C" uint32_t cornetto_qual_weight(int q) { return qm_e(q); }
