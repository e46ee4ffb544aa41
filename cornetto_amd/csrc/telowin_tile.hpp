// telowin_tile.hpp — the mark count of one 1000/200 window, shared by tw_scan (telo.hip: the windows themselves) and te_qual
// (telostats.hip: one qualification bit per window).  A workgroup of 256 threads owns a tile of 256 window starts of one contig; a window
// is five blocks of 200 bases (the last ones clipped at the contig's end, src/telomere_windows.c:36), so the workgroup counts its 260
// blocks ONCE (4-5 bitmap words each) and a window adds five counts — the first version counted the 16-17 words of every window per
// thread: 0.11 G wave-instructions per 3.16 Gbp step, a quarter of that now.
#pragma once
#include "common.hpp"

namespace cntw {
namespace {   // internal linkage: every translation unit that includes this gets its own copy

constexpr int TW_TILE = 256;            // window starts per tile (= threads of the workgroup)
constexpr int TW_BLOCKS = TW_TILE + 4;  // blocks of 200 bases its windows reach
constexpr int TW_WORDS = 816;           // the workgroup's 260 blocks of marks: 52 000 bits from any bit of a word

struct Window {
    bool visited;       // the loop of src/telomere_windows.c:31-41 comes by this window
    int start, end;     // [start, end): end - start = den (:36)
    int car;            // marked bases in it
};

__device__ __forceinline__ int popc_range(const unsigned long long *bm, long long a, long long b)
{
    int c = 0;
    while (a < b) {
        const long long wi = a >> 6;
        const int lo = (int)(a & 63);
        const long long wend = (wi + 1) << 6;
        const int hi = (int)((b < wend ? b : wend) - (wi << 6));
        const unsigned long long m = (hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
        c += __popcll(bm[wi] & m);
        a = wend;
    }
    return c;
}

// window tile.y + threadIdx.x of contig tile.x (length len, marks from bit boff of the bitmap); bc[TW_BLOCKS] and sw[TW_WORDS] are the
// workgroup's LDS.  Every thread of the workgroup calls it (two barriers inside).
__device__ __forceinline__ Window tile_window(const unsigned long long *bitmap, long long boff, int len, int2 tile, int *bc, unsigned long long *sw)
{
    // the words once, side by side (round 5; before: every thread its own 4-5 words one after the other — a chain of dependent round trips
    // to memory per workgroup, 0.166 ms for 0.4 GB; 0.138 now), the counts from LDS
    const long long bit0 = boff + (long long)tile.y * 200, bit1 = boff + len < bit0 + TW_BLOCKS * 200 ? boff + len : bit0 + TW_BLOCKS * 200;
    const long long w0 = bit0 >> 6;
    const int nw = bit1 > bit0 ? (int)(((bit1 + 63) >> 6) - w0) : 0;
    for (int k = threadIdx.x; k < nw; k += TW_TILE) sw[k] = bitmap[w0 + k];
    __syncthreads();
    for (int k = threadIdx.x; k < TW_BLOCKS; k += TW_TILE) {
        const long long lo = ((long long)tile.y + k) * 200;
        const long long hi = lo + 200 < len ? lo + 200 : len;
        bc[k] = lo < hi ? popc_range(sw, boff + lo - (w0 << 6), boff + hi - (w0 << 6)) : 0;
    }
    __syncthreads();
    const long long j = (long long)tile.y + threadIdx.x;
    const long long i = j * 200;                                   // WINDOW_SIZE / 5, :31
    Window w{false, 0, 0, 0};
    // the loop of :31-41 visits i = 0, 200, ... up to and including the first i with i + 1000 >= len
    if (i > len) return w;
    if (i > 0 && (i - 200) + 1000 >= len) return w;
    const int t = threadIdx.x;
    w.visited = true;
    w.start = (int)i;
    w.end = (int)((i + 1000 < len) ? i + 1000 : len);              // :36
    w.car = bc[t] + bc[t + 1] + bc[t + 2] + bc[t + 3] + bc[t + 4];
    return w;
}

}  // namespace
}  // namespace cntw
