// marks.hpp — the positions of the marked bytes of a text on the device, in order: the token starts of a bedgraph (bgtok.hpp), the
// newlines of a FASTA / FASTQ piece (fastq.hip).  What marks a byte is the caller's: a function that gives the mark bits of the
// 16 bytes at `pos` (bit i = byte pos + i; nothing at or beyond n).  Two kernels, 16 bytes per thread, ~1 B/byte read each:
// marks per tile of 4096 bytes -> scan of the tile counts (scan.hpp) -> ordered scatter of the positions.
#pragma once
#include "common.hpp"
#include "scan.hpp"

namespace cnmarks {
namespace {   // internal linkage: every translation unit that includes this gets its own copy

constexpr int MK_THREADS = 256;
constexpr int MK_TILE = MK_THREADS * 16;           // bytes of a tile

typedef uint32_t (*Mask16)(const uint8_t *text, int64_t pos, int64_t n);

template <Mask16 MASK>
__global__ __launch_bounds__(MK_THREADS) void mark_count(const uint8_t *text, int64_t n, uint32_t *tile_cnt)
{
    __shared__ uint32_t w[MK_THREADS / 64];
    const int64_t pos = ((int64_t)blockIdx.x * MK_THREADS + threadIdx.x) * 16;
    const uint32_t c = cnwave::wave_sum(pos < n ? (uint32_t)__popc(MASK(text, pos, n)) : 0u);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

// marks of the text in front of the 16 bytes of this thread, whose mark bits are m (tile_off: the scanned tile counts)
__device__ __forceinline__ uint32_t mark_rank(uint32_t m, const uint32_t *tile_off)
{
    uint32_t tile_total;
    return tile_off[blockIdx.x] + cnscan::block_excl<uint32_t, MK_THREADS>((uint32_t)__popc(m), tile_total);
}

template <Mask16 MASK>
__global__ __launch_bounds__(MK_THREADS) void mark_scatter(const uint8_t *text, int64_t n, const uint32_t *tile_off, uint32_t *out)
{
    const int64_t pos = ((int64_t)blockIdx.x * MK_THREADS + threadIdx.x) * 16;
    uint32_t m = pos < n ? MASK(text, pos, n) : 0u;
    uint32_t idx = mark_rank(m, tile_off);
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1;
        out[idx++] = (uint32_t)(pos + b);
    }
}

struct Marks {
    const uint32_t *tile_off;   // [nt] marks in front of every tile
    int64_t nt, total;
    uint8_t *extra;             // the caller's `extra_bytes` behind the counts (8-byte aligned, not initialised)
};

// Counts the marks of d_text[0, n), n > 0 (launch labels l_count, l_scan) in work space slot `slot`, and waits for the total.
template <Mask16 MASK>
int count(cornetto_accel_t *h, const char *who, const char *l_count, const char *l_scan, const uint8_t *d_text, int64_t n, int slot, size_t extra_bytes,
          Marks *mk)
{
    const int64_t nt = (n + MK_TILE - 1) / MK_TILE;
    // counts [nt] | offsets [nt] | (to a multiple of 8) total u64 | extra
    const size_t tot_at = ((size_t)2 * nt * 4 + 7) & ~(size_t)7;
    uint8_t *ws = (uint8_t *)cn_ws(h, slot, tot_at + 8 + extra_bytes);
    unsigned long long *p_tot = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!ws || !p_tot) return cn_fail(h, CORNETTO_E_NOMEM, "%s: workspace allocation failed", who);
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(ws), *d_off = d_cnt + nt;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(ws + tot_at);
    CN_LAUNCH(h, l_count, mark_count<MASK><<<dim3((unsigned)nt), dim3(MK_THREADS), 0, h->stream>>>(d_text, n, d_cnt));
    CN_TRY(cnscan::exclusive_u32(h, l_scan, d_cnt, nt, 1, d_off, d_tot));
    CN_HIP(h, hipMemcpyAsync(p_tot, d_tot, 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    *mk = Marks{d_off, nt, (int64_t)p_tot[0], ws + tot_at + 8};
    return CORNETTO_OK;
}

// The mk.total positions, in order, into work space slot `slot` (launch label l_scatter); nothing is launched when there is no mark.
template <Mask16 MASK>
int scatter(cornetto_accel_t *h, const char *who, const char *l_scatter, const uint8_t *d_text, int64_t n, const Marks &mk, int slot, size_t room,
            uint32_t **out)
{
    uint32_t *d_pos = (uint32_t *)cn_ws(h, slot, (room + 8) * 4);
    if (!d_pos) return cn_fail(h, CORNETTO_E_NOMEM, "%s: workspace allocation failed", who);
    if (mk.total) CN_LAUNCH(h, l_scatter, mark_scatter<MASK><<<dim3((unsigned)mk.nt), dim3(MK_THREADS), 0, h->stream>>>(d_text, n, mk.tile_off, d_pos));
    *out = d_pos;
    return CORNETTO_OK;
}

}  // namespace
}  // namespace cnmarks
