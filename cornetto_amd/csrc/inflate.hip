// inflate.hip — a BGZF-compressed text inflated on the device (include/cornetto_accel.h: cornetto_bgzf_scan, cornetto_text_inflate,
// cornetto_text_gather).  BGZF is a chain of independent gzip members of at most 64 KiB whose compressed size stands in the header and
// whose CRC-32 and size stand in the footer: the host walks the chain (inflate.hpp: cni_bgzf_scan), the device decodes a block per wave.
//   bgzf_inflate   the deflate decoder of inflate.hpp with the wave as its 64 lanes: bit buffer and symbol loop wave-uniform, tables
//                  built by the lanes in 3.8 KiB of LDS, literals gathered into wave-wide stores, matches and stored runs copied by the
//                  lanes.  A match reads bytes that other lanes of the wave stored: they are ordered by workgroup-scope release /
//                  acquire fences, set only where the match reaches behind the last fence.
//   bgzf_crc32     CRC-32 of every decoded block (64 slices, put together by multiplication with x^(8 len) mod P) against the footer;
//                  the lowest bad block's index is the call's answer.
//   text_gather    ranges of a device text packed back to back (the record names of an inflated FASTA text).
#include "common.hpp"
#include "inflate.hpp"
#include "internal.hpp"

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
    __device__ static void put(uint8_t *lit, int lane, uint8_t v)
    {
        if ((int)(threadIdx.x & 63) == lane) lit[0] = v;
    }
};

// one wave (= one workgroup) per block
__global__ void __launch_bounds__(64) bgzf_inflate(const uint8_t *__restrict__ comp, uint8_t *out, const cornetto_bgzf_block_t *__restrict__ blk, int64_t n_blk,
                                                   int32_t *__restrict__ status)
{
    __shared__ CniShared sh;
    const int64_t b = blockIdx.x;
    if (b >= n_blk) return;
    const cornetto_bgzf_block_t B = blk[b];
    const int st = cni_inflate<WaveLanes>(comp + B.src, B.n_src, out + B.dst, B.n_dst, sh);
    if (threadIdx.x == 0) status[b] = st;
}

__global__ void __launch_bounds__(64) bgzf_crc32(const uint8_t *__restrict__ out, const cornetto_bgzf_block_t *__restrict__ blk, int64_t n_blk, int32_t *status,
                                                 unsigned int *first_bad)
{
    __shared__ uint32_t tab[4 * 256], red[64];
    const int64_t b = blockIdx.x;
    if (b >= n_blk) return;
    const cornetto_bgzf_block_t B = blk[b];
    int st = status[b];
    if (st == CNI_OK && cni_crc32<WaveLanes>(out + B.dst, B.n_dst, tab, red) != B.crc) st = CNI_BAD_CRC;
    if (threadIdx.x == 0 && st != CNI_OK) {
        status[b] = st;
        atomicMin(first_bad, (unsigned int)b);
    }
}

// a thread per packed byte: the range it belongs to by bisection of the ranges' packed offsets to[0 .. n]
__global__ void __launch_bounds__(256) text_gather(const uint8_t *__restrict__ text, const int64_t *__restrict__ at, const int64_t *__restrict__ to, int64_t n,
                                                   int64_t total, uint8_t *__restrict__ pack)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    int64_t lo = 0, hi = n - 1;          // the last range with to[i] <= j (empty ranges in front of it share its offset)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (to[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    pack[j] = text[at[lo] + (j - to[lo])];
}

}   // namespace

// The two kernels over raw device pointers (internal.hpp): what cornetto_text_inflate() runs between its checks and its timing bracket, and what
// the bedgraph feeds run into their own text workspaces.  The caller has checked that every block lies inside both buffers and that the
// compressed bytes are on the device.  Synchronises the handle's stream.  *first_bad: -1, or the lowest index of a bad block.
int cn_bgzf_inflate_raw(cornetto_accel_t *h, const uint8_t *d_comp, uint8_t *d_out, const cornetto_bgzf_block_t *blocks, int64_t n_blocks, int64_t *first_bad)
{
    *first_bad = -1;
    if (n_blocks <= 0) return CORNETTO_OK;
    cornetto_bgzf_block_t *d_blk = (cornetto_bgzf_block_t *)cn_ws(h, WS_BZ_BLOCKS, (size_t)n_blocks * sizeof(cornetto_bgzf_block_t));
    int32_t *d_st = (int32_t *)cn_ws(h, WS_BZ_STATUS, ((size_t)n_blocks + 4) * 4);
    unsigned int *p_bad = (unsigned int *)cn_pin(h, PIN_SMALL, 64);
    if (!d_blk || !d_st || !p_bad) return cn_fail(h, CORNETTO_E_NOMEM, "text_inflate: workspace allocation failed");
    unsigned int *d_bad = (unsigned int *)(d_st + n_blocks);
    CN_HIP(h, hipMemcpyAsync(d_blk, blocks, (size_t)n_blocks * sizeof(cornetto_bgzf_block_t), hipMemcpyHostToDevice, h->stream));
    CN_HIP(h, hipMemsetAsync(d_bad, 0xFF, 4, h->stream));
    CN_LAUNCH(h, "bgzf_inflate", bgzf_inflate<<<dim3((unsigned)n_blocks), dim3(64), 0, h->stream>>>(d_comp, d_out, d_blk, n_blocks, d_st));
    CN_LAUNCH(h, "bgzf_crc32", bgzf_crc32<<<dim3((unsigned)n_blocks), dim3(64), 0, h->stream>>>(d_out, d_blk, n_blocks, d_st, d_bad));
    CN_HIP(h, hipMemcpyAsync(p_bad, d_bad, 4, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    if (p_bad[0] != 0xFFFFFFFFu) *first_bad = (int64_t)p_bad[0];
    return CORNETTO_OK;
}

extern "C" int cornetto_bgzf_scan(const uint8_t *buf, int64_t n, int64_t file_off, int64_t *dst, cornetto_bgzf_block_t *blocks, int64_t cap, int64_t *n_blocks,
                                  int64_t *resume, int32_t *broken)
{
    if (n < 0 || (n > 0 && !buf) || file_off < 0 || !dst || cap < 0 || (cap > 0 && !blocks) || !n_blocks || !resume || !broken) return CORNETTO_E_ARG;
    return cni_bgzf_scan(buf, n, file_off, dst, blocks, cap, n_blocks, resume, broken);
}

extern "C" int cornetto_text_inflate(cornetto_accel_t *h, cornetto_text_t *comp, cornetto_text_t *out, const cornetto_bgzf_block_t *blocks, int64_t n_blocks,
                                     int64_t *first_bad)
{
    if (!h || !comp || !out || comp == out || n_blocks < 0 || n_blocks > 0x7fffffffLL || (n_blocks > 0 && !blocks) || !first_bad)
        return cn_fail(h, CORNETTO_E_ARG, "text_inflate: bad argument");
    *first_bad = -1;
    for (int64_t i = 0; i < n_blocks; ++i) {
        const cornetto_bgzf_block_t &b = blocks[i];
        if (b.src < 0 || b.n_src < 0 || b.src > comp->cap - b.n_src || b.dst < 0 || b.n_dst < 0 || b.n_dst > 65536 || b.dst > out->cap - b.n_dst)
            return cn_fail(h, CORNETTO_E_ARG, "text_inflate: block %lld lies outside its text", (long long)i);
    }
    if (n_blocks == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    for (int i = 0; i < 4; ++i) CN_HIP(h, hipStreamSynchronize(comp->q[i]));     // every slab is on the device
    cn_timing_begin(h);
    CN_TRY(cn_bgzf_inflate_raw(h, comp->d, out->d, blocks, n_blocks, first_bad));
    cn_timing_end(h);
    if (*first_bad >= 0) return cn_fail(h, CORNETTO_E_FORMAT, "text_inflate: block %lld is not what its footer says", (long long)*first_bad);
    return CORNETTO_OK;
}

extern "C" int cornetto_text_gather(cornetto_accel_t *h, cornetto_text_t *t, const int64_t *at, const int32_t *len, int64_t n, char *dst)
{
    if (!h || !t || n < 0 || (n > 0 && (!at || !len))) return cn_fail(h, CORNETTO_E_ARG, "text_gather: bad argument");
    if (n == 0) return CORNETTO_OK;
    std::vector<int64_t> tab;
    tab.reserve((size_t)(2 * n + 1));
    for (int64_t i = 0; i < n; ++i) {
        if (at[i] < 0 || len[i] < 0 || at[i] > t->cap - len[i]) return cn_fail(h, CORNETTO_E_ARG, "text_gather: range %lld lies outside the text", (long long)i);
        tab.push_back(at[i]);
    }
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        tab.push_back(total);
        total += len[i];
    }
    tab.push_back(total);
    if (total == 0) return CORNETTO_OK;
    if (total > 0xFFFFFF00LL) return cn_fail(h, CORNETTO_E_ARG, "text_gather: more than a text of bytes");
    if (!dst) return cn_fail(h, CORNETTO_E_ARG, "text_gather: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    for (int i = 0; i < 4; ++i) CN_HIP(h, hipStreamSynchronize(t->q[i]));
    cn_timing_begin(h);
    int64_t *d_tab = (int64_t *)cn_ws(h, WS_BZ_BLOCKS, tab.size() * 8);
    uint8_t *d_pack = (uint8_t *)cn_ws(h, WS_BZ_PACK, (size_t)total);
    if (!d_tab || !d_pack) return cn_fail(h, CORNETTO_E_NOMEM, "text_gather: workspace allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, h->stream));
    CN_LAUNCH(h, "text_gather", text_gather<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream>>>(t->d, d_tab, d_tab + n, n, total, d_pack));
    CN_HIP(h, hipMemcpyAsync(dst, d_pack, (size_t)total, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    return CORNETTO_OK;
}
