// scan.hpp — device-wide exclusive prefix sum of 32-bit counters (strided input), used to turn per-tile /
// per-chunk counts into ordered output offsets without a host round trip.  ONE launch (round 4; three before: tile-local scan,
// scan of the tile totals, offset add — at a 395 Mb share a step is made of such launches, ~10 us of stream time each): every
// workgroup scans its 4096 items, publishes its total, and looks back over the states of the tiles in front of it until it meets
// one whose inclusive prefix is known ("decoupled look-back").  A tile's number is the order in which it STARTED (a ticket), so
// everything it waits for is already running.  The pieces (the scan inside a tile, the look-back) are device functions: the 64-bit
// scan of bgrun.hip and the head count of ivlmerge.hpp's fused merge are built from the same ones.
#pragma once
#include "common.hpp"
#include "wave.hpp"

namespace cnscan {
namespace {   // internal linkage: every translation unit that includes this gets its own copy

constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS = 16;                       // per thread
constexpr int SC_TILE = SC_THREADS * SC_ITEMS;     // 4096

// One value per thread of a workgroup of THREADS -> the sum over the threads in front of it; total = the sum over all of them.
// (Holds a barrier and the workgroup's wave totals: once per kernel.)
template <typename T, int THREADS>
__device__ __forceinline__ T block_excl(T s, T &total)
{
    __shared__ T wtot[THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T inc = cnwave::wave_incl(s, lane);
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    T pre = inc - s;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        if (w < wv) pre += wtot[w];
        total += wtot[w];
    }
    return pre;
}

// The scan inside a tile of SC_THREADS * ITEMS values: v[k] = in[(base + k) * stride] (0 at and beyond n), returns the sum of the tile's
// values in front of v[0]; total = the tile's sum.
template <typename T, int ITEMS>
__device__ __forceinline__ T tile_excl(const T *in, int64_t base, int64_t n, int stride, T (&v)[ITEMS], T &total)
{
    T s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = base + k;
        v[k] = i < n ? in[i * stride] : (T)0;
        s += v[k];
    }
    return block_excl<T, SC_THREADS>(s, total);
}

// out[base + k] = pre + v[0] + ... + v[k - 1]
template <typename T, int ITEMS>
__device__ __forceinline__ void tile_write(T *out, int64_t base, int64_t n, T pre, const T (&v)[ITEMS])
{
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = base + k;
        if (i < n) out[i] = pre;
        pre += v[k];
    }
}

// ---- decoupled look-back ------------------------------------------------------------------------------------------------------
// state of a tile: [63:62] 1 = the tile's own total, 2 = the inclusive prefix up to and including it; [61:32] the epoch of the call
// that wrote it; [31:0] the value.  The state of tile t lives at st[t * stride].  States are never cleared: a word of another epoch
// is "not written yet".
//
// Called by the first wave of tile `tile` with the tile's own total: returns the sum of the totals of the tiles in front of it.
// Publish the own total, poll 64 predecessors per round, stop at the nearest one whose inclusive prefix is known, publish the
// inclusive prefix.  Why the wait ends, and what therefore stays as it is:
//   - `tile` is a TICKET, the order in which the workgroups started: every tile polled here is running already, whatever order the
//     hardware hands out block indices in;
//   - the own total is published BEFORE the wait and the inclusive prefix after it: a running tile owes its total to nobody (tile 0
//     waits for nobody), so every poll meets at least totals, and the prefix of the nearest finished tile cuts the walk short;
//   - the polls are relaxed atomic loads at agent scope: issued again in every round (nothing the compiler may keep in a register)
//     and served where the stores of the other compute units arrive; the value travels in the state word itself, so no fence;
//   - s_sleep(1) between two polls leaves the issue slots to the waves that still have their totals to compute.
__device__ __forceinline__ uint32_t lookback_excl(unsigned long long *st, int64_t stride, int64_t tile, uint32_t epoch, uint32_t own, int lane)
{
    const unsigned long long tag = (unsigned long long)(epoch & 0x3FFFFFFFu) << 32;
    uint32_t excl = 0;
    if (tile > 0) {
        if (lane == 0) __hip_atomic_store(&st[tile * stride], (1ull << 62) | tag | own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int64_t pos = tile - 1;; pos -= 64) {
            const int64_t idx = pos - lane;
            unsigned long long x;
            for (;;) {
                x = idx >= 0 ? __hip_atomic_load(&st[idx * stride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((2ull << 62) | tag);
                const bool ready = (x >> 62) != 0 && (x & (0x3FFFFFFFull << 32)) == tag;
                if (__builtin_amdgcn_ballot_w64(!ready) == 0) break;
                __builtin_amdgcn_s_sleep(1);
            }
            const unsigned long long incl = __builtin_amdgcn_ballot_w64((x >> 62) == 2);
            const uint32_t val = (uint32_t)x;
            if (incl) {
                const int first = __builtin_ctzll(incl);          // the nearest tile whose prefix is complete
                excl += cnwave::wave_sum(lane <= first ? val : 0u);
                break;
            }
            excl += cnwave::wave_sum(val);
        }
    }
    if (lane == 0) __hip_atomic_store(&st[tile * stride], (2ull << 62) | tag | (excl + own), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// Up to four counters that sit side by side in one record (in[i * stride + q], q < m) are scanned by one launch (a 395 Mb share is made
// of launches: 12 -> 3 -> 1 in front of telofind's gather): tile t of counter q draws the ticket q * np + t.
struct Outs4 {
    uint32_t *o[4];
};
struct LbArgs {
    const uint32_t *in;
    int64_t n, np;
    int stride, m;
    Outs4 outs;
    unsigned long long *state;     // [m * np]
    uint32_t *ticket;
    uint32_t ticket_base, epoch;
    unsigned long long *total;     // [m] or null
};

__global__ __launch_bounds__(SC_THREADS) void scan_lookback(LbArgs A)
{
    __shared__ uint32_t s_gid, s_excl;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) s_gid = atomicAdd(A.ticket, 1u) - A.ticket_base;
    __syncthreads();
    const int64_t gid = s_gid;
    if (gid >= (int64_t)A.m * A.np) return;          // (a ticket base out of step with the counter — the host resets both on any error: never an index)
    const int q = (int)(gid / A.np);
    const int64_t tile = gid - (int64_t)q * A.np;
    const int64_t base = tile * SC_TILE + (int64_t)t * SC_ITEMS;
    uint32_t v[SC_ITEMS], bt;
    uint32_t pre = tile_excl(A.in + q, base, A.n, A.stride, v, bt);
    if (wv == 0) {
        const uint32_t excl = lookback_excl(A.state + (int64_t)q * A.np, 1, tile, A.epoch, bt, lane);
        if (lane == 0) {
            s_excl = excl;
            if (A.total && tile == A.np - 1) A.total[q] = (unsigned long long)excl + bt;
        }
    }
    __syncthreads();
    pre += s_excl;
    tile_write(A.outs.o[q], base, A.n, pre, v);
}

// outs[q][i] = exclusive prefix of in[i * stride + q] for q < m (<= 4); d_total (optional): m grand totals (u64 each).
// The contract of the 32-bit arithmetic: the offsets are the prefixes mod 2^32 — exact as long as the sum of everything in front of an
// item is below 2^32 —, and a grand total is (u64)(exclusive prefix of the last tile, 32 bits) + the last tile's sum (32 bits): exact
// only while the sum of all items is below 2^32, and never above 2^33 - 2.  Every caller bounds its sum by what it counts (DESIGN 4.3:
// the table of call sites); nothing here checks it.
static inline int exclusive_u32_multi(cornetto_accel_t *h, const char *name, const uint32_t *in, int64_t n, int stride, int m, uint32_t *const *outs,
                                      unsigned long long *d_total)
{
    if (n <= 0 || m <= 0) return CORNETTO_OK;
    if (m > 4) m = 4;
    Outs4 o{};
    for (int q = 0; q < m; ++q) o.o[q] = outs[q];
    const int64_t np = (n + SC_TILE - 1) / SC_TILE;
    const size_t need = 64 + (size_t)m * (size_t)np * 8;
    // (the epoch has 30 bits in a state: after the last one the states are cleared like new memory — epoch 1 of the next round would
    // otherwise meet the words that the first epoch 1 left in the tiles no call since has reached, and take them for prefixes)
    const bool fresh = h->dev[WS_SCAN].bytes < need || h->scan_epoch >= 0x3FFFFFFFu;
    uint8_t *ws = (uint8_t *)cn_ws(h, WS_SCAN, need);
    if (!ws) return cn_fail(h, CORNETTO_E_NOMEM, "scan: workspace allocation failed");
    const int rc = [&]() -> int {
        if (fresh) {                                 // new memory, or every epoch used: no state of any epoch in it, the ticket counter starts again
            CN_HIP(h, hipMemsetAsync(ws, 0, h->dev[WS_SCAN].bytes, h->stream));
            h->scan_tickets = 0;
            h->scan_epoch = 0;
        }
        const uint32_t epoch = h->scan_epoch + 1;    // 1 .. 0x3FFFFFFF
        LbArgs A{in, n, np, stride, m, o, reinterpret_cast<unsigned long long *>(ws + 64), reinterpret_cast<uint32_t *>(ws), h->scan_tickets, epoch, d_total};
        CN_LAUNCH(h, name, scan_lookback<<<dim3((unsigned)(m * np)), dim3(SC_THREADS), 0, h->stream>>>(A));
        h->scan_epoch = epoch;                       // the device's ticket counter advances iff the kernel was queued: the host's copy only then
        h->scan_tickets += (uint32_t)(m * np);
        return CORNETTO_OK;
    }();
    if (rc != CORNETTO_OK) h->dev[WS_SCAN].bytes = 0;   // counters possibly out of step: the next call gets new, cleared memory (cn_ws frees the block)
    return rc;
}

// out[i] (u32) = exclusive prefix of in[i*stride]; d_total (optional, device u64) = grand total.
static inline int exclusive_u32(cornetto_accel_t *h, const char *name, const uint32_t *in, int64_t n, int stride, uint32_t *out, unsigned long long *d_total)
{
    return exclusive_u32_multi(h, name, in, n, stride, 1, &out, d_total);
}

}  // namespace
}  // namespace cnscan
