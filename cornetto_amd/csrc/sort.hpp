// sort.hpp — stable device sort of (64-bit key, 32-bit payload) pairs: least-significant-digit radix sort, 8 bits per pass, for gfx950.
// The interval stages before this one (ivlmerge.hpp, cov.hip, telostats.hip) get their input in (contig, start) order or sort on the host
// (panel.hip); PAF rows come in no useful order (hap.hip), so the order is made here, without a host round trip inside: n is the host's.
//
// One pass over digit d = (key >> shift) & 255, a tile = SO_TILE consecutive pairs, one pair per thread:
//   so_hist     every tile counts its keys per digit value -> table[v * tiles + tile] (bin-major: the exclusive scan of the table in
//               this order IS the first output index of (value v, tile t) — all smaller values first, then the tiles in front);
//   the scan    cnscan::exclusive_u32 over the 256 * tiles counters (scan.hpp: one launch);
//   so_scatter  every pair goes to table'[v][tile] + its rank among the pairs of the tile with the same digit value, in input order.
// The rank is what makes a pass stable.  Inside a wave: eight ballots, one per digit bit, leave every lane with the 64-bit mask of the
// lanes that hold its digit value (lanes behind the end of the input are in no mask); the rank in the wave is the number of set bits
// below the lane, the lowest lane of a mask stores the mask's population as the wave's count of that value.  Across the waves of the
// workgroup: thread v turns the column of value v into the counts of the waves in front.  No atomic anywhere: the same input gives the
// same output bit for bit, whatever order the workgroups run in.
// Digits at and above key_bits are not touched (the keys are zero there by contract): ceil(key_bits / 8) passes, ping-pong between the
// caller's arrays and a second pair in the workspace; the caller is told where the result ended.
#pragma once
#include "common.hpp"
#include "scan.hpp"

namespace cnsort {
namespace {

constexpr int SO_THREADS = 1024, SO_WAVES = SO_THREADS / 64;
constexpr int SO_TILE = SO_THREADS;                // one pair per thread (uncoalesced scatter writes are accepted at these sizes)

// -> the mask of the lanes of this wave that hold `digit` among the lanes with valid = true (0 for a lane that is not valid)
__device__ __forceinline__ unsigned long long so_match(uint32_t digit, bool valid)
{
    unsigned long long m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(bit);
        m &= bit ? bal : ~bal;
    }
    return valid ? m : 0ull;
}

// wcnt[w][v] = pairs of wave w with digit value v (every thread of the workgroup calls it; ends with a barrier)
__device__ __forceinline__ void so_wave_counts(uint32_t (*wcnt)[256], unsigned long long mask, uint32_t digit, int lane, int wv)
{
    for (int i = threadIdx.x; i < SO_WAVES * 256; i += SO_THREADS) (&wcnt[0][0])[i] = 0u;
    __syncthreads();
    if (mask && lane == __builtin_ctzll(mask)) wcnt[wv][digit] = (uint32_t)__popcll(mask);
    __syncthreads();
}

__global__ __launch_bounds__(SO_THREADS) void so_hist(const unsigned long long *keys, int64_t n, int shift, int64_t tiles, uint32_t *table)
{
    __shared__ uint32_t wcnt[SO_WAVES][256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * SO_TILE + t;
    const bool valid = i < n;
    const uint32_t digit = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
    so_wave_counts(wcnt, so_match(digit, valid), digit, lane, wv);
    if (t < 256) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < SO_WAVES; ++w) s += wcnt[w][t];
        table[(int64_t)t * tiles + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(SO_THREADS) void so_scatter(const unsigned long long *keys, const uint32_t *vals, int64_t n, int shift, int64_t tiles,
                                                         const uint32_t *first, unsigned long long *out_keys, uint32_t *out_vals)
{
    __shared__ uint32_t wcnt[SO_WAVES][256];
    __shared__ uint32_t base[256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * SO_TILE + t;
    const bool valid = i < n;
    const unsigned long long key = valid ? keys[i] : 0ull;
    const uint32_t val = valid ? vals[i] : 0u;
    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
    const unsigned long long mask = so_match(digit, valid);
    so_wave_counts(wcnt, mask, digit, lane, wv);
    if (t < 256) {                                     // the column of value t: counts -> counts of the waves in front
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < SO_WAVES; ++w) {
            const uint32_t c = wcnt[w][t];
            wcnt[w][t] = s;
            s += c;
        }
        base[t] = first[(int64_t)t * tiles + blockIdx.x];
    }
    __syncthreads();
    if (!valid) return;
    const int64_t pos = (int64_t)base[digit] + wcnt[wv][digit] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (pos < n) {                                     // (always, with a table that was scanned: never an index beyond the arrays)
        out_keys[pos] = key;
        out_vals[pos] = val;
    }
}

static inline int64_t n_tiles(int64_t n) { return (n + SO_TILE - 1) / SO_TILE; }

// bytes of device workspace pairs_u64() needs for n pairs: the second pair of arrays, the table and its scan
static inline size_t ws_bytes(int64_t n)
{
    const size_t m = (size_t)(n > 0 ? n : 1), tab = 256 * (size_t)n_tiles(n > 0 ? n : 1);
    return cn_align_up((int64_t)(m * 8), 256) + cn_align_up((int64_t)(m * 4), 256) + 2 * cn_align_up((int64_t)(tab * 4), 256);
}

// Sorts d_keys[0 .. n) ascending, stable, d_vals going with them; only the digits below key_bits (1 .. 64) are looked at, the keys are 0
// above.  ws: ws_bytes(n) bytes, 256-byte aligned.  *out_keys / *out_vals: where the sorted pairs are (the caller's arrays or the
// workspace's, by the parity of the number of passes); the other pair of arrays holds the last pass's input.
static inline int pairs_u64(cornetto_accel_t *h, const char *name, unsigned long long *d_keys, uint32_t *d_vals, int64_t n, uint8_t *ws, int key_bits,
                            unsigned long long **out_keys, uint32_t **out_vals)
{
    *out_keys = d_keys;
    *out_vals = d_vals;
    if (n <= 1) return CORNETTO_OK;
    if (key_bits < 1 || key_bits > 64) return cn_fail(h, CORNETTO_E_ARG, "%s: %d key bits", name, key_bits);
    // (the table's scan is 32-bit: exact while n < 2^32, scan.hpp; a grid has 2^31 - 1 workgroups)
    if (n > 0x7FFFFFFFll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "%s: %lld pairs, at most 2^31-1 are sorted in one call", name, (long long)n);
    const int64_t tiles = n_tiles(n), tab = 256 * tiles;
    unsigned long long *k[2] = {d_keys, reinterpret_cast<unsigned long long *>(ws)};
    uint32_t *v[2] = {d_vals, reinterpret_cast<uint32_t *>(ws + cn_align_up(n * 8, 256))};
    uint32_t *table = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(v[1]) + cn_align_up(n * 4, 256));
    uint32_t *first = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(table) + cn_align_up(tab * 4, 256));
    int cur = 0;
    for (int shift = 0; shift < key_bits; shift += 8, cur ^= 1) {
        CN_LAUNCH(h, name, so_hist<<<dim3((unsigned)tiles), dim3(SO_THREADS), 0, h->stream>>>(k[cur], n, shift, tiles, table));
        CN_TRY(cnscan::exclusive_u32(h, name, table, tab, 1, first, nullptr));
        CN_LAUNCH(h, name, so_scatter<<<dim3((unsigned)tiles), dim3(SO_THREADS), 0, h->stream>>>(k[cur], v[cur], n, shift, tiles, first, k[cur ^ 1], v[cur ^ 1]));
    }
    *out_keys = k[cur];
    *out_vals = v[cur];
    return CORNETTO_OK;
}

}  // namespace
}  // namespace cnsort
