// deflate.hip — a device text deflated into BGZF members on the device (include/cornetto_accel.h: cornetto_text_deflate; bamfq.hip runs the
// same kernels over the slab bamfq_text has written: cornetto_bamfq_get_bgzf).  The text is cut every CND_MEMBER bytes:
//   bgzf_deflate   the encoder of deflate.hpp with the wave as its 64 lanes, a wave (= a workgroup) per member, 14.5 KiB of LDS: run flags by
//                  ballot, the histogram with equal symbols of the wave added once, Huffman lengths, the code stream ORed into zeroed LDS
//                  words at the offsets of a wave prefix sum, the CRC-32 of inflate.hpp; the member goes to staging of a fixed stride
//   bgzf_scan      (scan.hpp) the members' sizes -> their offsets in the packed chain, and its length
//   bgzf_pack      a workgroup per member: its bytes from staging to their place, aligned words of the destination
#include "common.hpp"
#include "deflate.hpp"
#include "internal.hpp"
#include "scan.hpp"
#include "wave.hpp"

namespace {

struct WaveLanes {
    static constexpr int SLOTS = 1;
    __device__ static int first() { return (int)(threadIdx.x & 63); }
    __device__ static int step() { return 64; }
    __device__ static int slot(int) { return 0; }
    __device__ static bool leader() { return (threadIdx.x & 63) == 0; }
    __device__ static void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ static int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
    __device__ static uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ static uint64_t ballot(const bool *f) { return __builtin_amdgcn_ballot_w64(f[0]); }
    __device__ static uint32_t scan(const uint32_t *v, uint32_t *ex)
    {
        const uint32_t inc = cnwave::wave_incl(v[0], (int)(threadIdx.x & 63));
        ex[0] = inc - v[0];
        return (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    __device__ static uint32_t pick(const uint32_t *v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v[0], __builtin_amdgcn_readfirstlane(lane & 63)); }
    __device__ static void lds_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    __device__ static void lds_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};

// one wave (= one workgroup) per member: bytes [m CND_MEMBER, min(n, (m + 1) CND_MEMBER)) of src -> stage + m CND_STRIDE, its size -> size[m]
__global__ void __launch_bounds__(64) bgzf_deflate(const uint8_t *__restrict__ src, int64_t n, uint8_t *__restrict__ stage, int64_t n_mem, uint32_t *__restrict__ size)
{
    __shared__ CndShared sh;
    const int64_t m = blockIdx.x;
    if (m >= n_mem) return;
    const int64_t at = m * CND_MEMBER, left = n - at;
    const int32_t len = left < 0 ? 0 : left < CND_MEMBER ? (int32_t)left : (int32_t)CND_MEMBER;
    const int32_t sz = cnd_member<WaveLanes>(src + at, len, stage + m * CND_STRIDE, sh);
    if (threadIdx.x == 0) size[m] = (uint32_t)sz;
}

__global__ void __launch_bounds__(256) bgzf_pack(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ size, const uint32_t *__restrict__ off, int64_t n_mem,
                                                 uint8_t *__restrict__ out)
{
    const int64_t m = blockIdx.x;
    if (m >= n_mem) return;
    const uint8_t *s = stage + m * CND_STRIDE + CND_HEAD;
    uint32_t n = size[m];
    if (n > (uint32_t)CND_MAX_SIZE) n = (uint32_t)CND_MAX_SIZE;      // (what the staging of a member holds at most)
    uint8_t *d = out + off[m];
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
    if (head > n) head = n;
    if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    const uint32_t words = (n - head) >> 2;
    for (uint32_t w = threadIdx.x; w < words; w += 256) {
        uint32_t v;
        memcpy(&v, s + head + 4 * w, 4);
        *reinterpret_cast<uint32_t *>(d + head + 4 * w) = v;
    }
    const uint32_t done = head + 4 * words;
    if (threadIdx.x < n - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

}   // namespace

// The three kernels over raw device pointers (internal.hpp), queued on the handle's stream; nothing is waited for.
int cn_bgzf_deflate_queue(cornetto_accel_t *h, const uint8_t *d_src, int64_t n, uint8_t *d_out, unsigned long long *d_total)
{
    const int64_t n_mem = (n + CND_MEMBER - 1) / CND_MEMBER;
    if (n_mem <= 0) {
        CN_HIP(h, hipMemsetAsync(d_total, 0, 8, h->stream));
        return CORNETTO_OK;
    }
    uint8_t *d_stage = (uint8_t *)cn_ws(h, WS_DF_STAGE, (size_t)n_mem * CND_STRIDE);
    uint32_t *d_size = (uint32_t *)cn_ws(h, WS_DF_SIZE, (size_t)n_mem * 8);
    if (!d_stage || !d_size) return cn_fail(h, CORNETTO_E_NOMEM, "text_deflate: workspace allocation failed (%lld members)", (long long)n_mem);
    uint32_t *d_off = d_size + n_mem;
    CN_LAUNCH(h, "bgzf_deflate", bgzf_deflate<<<dim3((unsigned)n_mem), dim3(64), 0, h->stream>>>(d_src, n, d_stage, n_mem, d_size));
    CN_TRY(cnscan::exclusive_u32(h, "bgzf_scan", d_size, n_mem, 1, d_off, d_total));
    CN_LAUNCH(h, "bgzf_pack", bgzf_pack<<<dim3((unsigned)n_mem), dim3(256), 0, h->stream>>>(d_stage, d_size, d_off, n_mem, d_out));
    return CORNETTO_OK;
}

extern "C" int cornetto_text_deflate(cornetto_accel_t *h, cornetto_text_t *text, int64_t at, int64_t n, cornetto_text_t *out, int64_t out_at, int64_t *n_out,
                                     int64_t *n_members)
{
    if (!h || !text || !out || text == out || !n_out || !n_members || at < 0 || n < 0 || n > 0xF0000000ll || at > text->cap - n || out_at < 0 || out_at > out->cap)
        return cn_fail(h, CORNETTO_E_ARG, "text_deflate: bad argument");
    const int64_t n_mem = (n + CND_MEMBER - 1) / CND_MEMBER;
    if (n_mem * CND_STRIDE > out->cap - out_at)
        return cn_fail(h, CORNETTO_E_ARG, "text_deflate: %lld members want room for %lld bytes, the text has %lld behind %lld", (long long)n_mem,
                       (long long)(n_mem * CND_STRIDE), (long long)(out->cap - out_at), (long long)out_at);
    *n_out = 0;
    *n_members = 0;
    if (n == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    for (int i = 0; i < 4; ++i) CN_HIP(h, hipStreamSynchronize(text->q[i]));     // every slab is on the device
    unsigned long long *d_tot = (unsigned long long *)cn_ws(h, WS_DF_TOTAL, 64);
    unsigned long long *p_tot = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!d_tot || !p_tot) return cn_fail(h, CORNETTO_E_NOMEM, "text_deflate: workspace allocation failed");
    cn_timing_begin(h);
    CN_TRY(cn_bgzf_deflate_queue(h, text->d + at, n, out->d + out_at, d_tot));
    CN_HIP(h, hipMemcpyAsync(p_tot, d_tot, 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    if (p_tot[0] > (unsigned long long)(n_mem * CND_MAX_SIZE)) return cn_fail(h, CORNETTO_E_HIP, "text_deflate: %llu bytes from %lld members", p_tot[0], (long long)n_mem);
    *n_out = (int64_t)p_tot[0];
    *n_members = n_mem;
    return CORNETTO_OK;
}
