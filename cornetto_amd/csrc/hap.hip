// hap.hip — cornetto_hap_fun(): the haplotype stage of the diploid panel, scripts/create-hapnetto.sh:40-67, for gfx950: from the rows of
// the haplotype-to-primary PAFs (query, target, start, end) to hap1_hap2_funbits.bed without cut / sort / awk / bedtools and without the
// shell loop that runs `bedtools sort | bedtools merge` once per haplotype contig.  The rows go up once, the merged funbits come back.
//
//   :48-51  blocks   rows sorted by (haplotype, query, target, start) — two chained stable radix sorts (sort.hpp): by target << 32 | start,
//                    then by haplotype << 32 | query —, the (haplotype, query, target) groups numbered by head flags and the add-scan
//                    (scan.hpp), cnivl::merge (ivlmerge.hpp) with the group number in place of the contig and dist = merge_dist
//   :58     corners  at most two per block, taken BEFORE the union across queries, compacted through a scan; not clamped to the contig
//                    (the script does not), capped at INT32_MAX as cornetto_panel_boring() caps
//   :55     gaps     blocks sorted by (haplotype, target, start), merged with 0; every contig of every haplotype minus that list: count,
//                    scan, write (a contig without blocks: its whole length; a contig of length 0: nothing; no zero-length row)
//   :61,67  funbits  gaps and corners of ALL haplotypes sorted by (target, start) and merged with 0 — merge(merge(A) + merge(B)) =
//                    merge(A + B), so one sort and one merge stand for the per-haplotype merges and the one across haplotypes.
// Three counts come back to the host on the way (blocks; corners and gaps; funbits): the sorts want their n from the host.
//
// PARITY UNPINNED, as for panel.hip: bedtools is not available where this was written; the semantics are those of the bedtools manual
// (merge -d: features at most d apart merge, book-ended ones included; subtract: the parts of A no B covers) and of the awk one-liners as
// written.  Stated divergences from the script:
//   - the intermediate funbits are ordered by (assembly-BED order, start), not by `bedtools sort`'s name order; the final panel comes out
//     in assembly order from `subtract -a` either way;
//   - names are compared as byte strings by the caller that makes the ids; awk's $1==ctg compares numeric-looking names as numbers;
//   - a PAF row whose target is not in the assembly BED never gets here: the caller drops and counts it;
//   - a row with end <= start or a negative coordinate is an error (CORNETTO_E_ARG);
//   - a haplotype without any row yields whole contigs as gaps here; the CLI refuses it (the script dies there too: it never creates
//     ${HAP}_tmp.bed).
#include <climits>

#include "common.hpp"
#include "ivlmerge.hpp"
#include "scan.hpp"
#include "sort.hpp"

namespace {

using u64 = unsigned long long;

// keys[i] = target << 32 | start, vals[i] = i
__global__ __launch_bounds__(256) void hp_key_pos(const cornetto_hap_row_t *rows, int64_t n, u64 *keys, uint32_t *vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((u64)(uint32_t)rows[i].ctg << 32) | (uint32_t)rows[i].start;
    vals[i] = (uint32_t)i;
}

// keys[j] = haplotype << 32 | query of row in_vals[j] (the haplotype of a row: its place among the prefix sums `pref` of the row counts),
// vals[j] = in_vals[j]; in_vals may be vals
__global__ __launch_bounds__(256) void hp_key_query(const cornetto_hap_row_t *rows, const uint32_t *in_vals, int64_t n, const int64_t *pref, int32_t n_hap, u64 *keys,
                                                    uint32_t *vals)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = in_vals[j];
    int32_t lo = 0, hi = n_hap - 1;                    // the last haplotype whose first row is at or before r
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (pref[mid] <= (int64_t)r) lo = mid;
        else hi = mid - 1;
    }
    keys[j] = ((u64)(uint32_t)lo << 32) | (uint32_t)rows[r].query;
    vals[j] = r;
}

// head[j] = 1 where the (haplotype, query, target) of sorted row j differs from the row in front
__global__ __launch_bounds__(256) void hp_heads(const cornetto_hap_row_t *rows, const u64 *keys, const uint32_t *vals, int64_t n, uint32_t *head)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || keys[j] != keys[j - 1] || rows[vals[j]].ctg != rows[vals[j - 1]].ctg) ? 1u : 0u;
}

// the sorted rows as intervals of their group; grp[g] = {haplotype, target} of group g
__global__ __launch_bounds__(256) void hp_groups(const cornetto_hap_row_t *rows, const u64 *keys, const uint32_t *vals, int64_t n, const uint32_t *head, const uint32_t *rank,
                                                 cornetto_ivl_t *ivl, int2 *grp)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const cornetto_hap_row_t r = rows[vals[j]];
    const uint32_t g = rank[j] + head[j] - 1u;         // heads before j, plus j itself when it is one
    ivl[j] = cornetto_ivl_t{(int32_t)g, r.start, r.finish};
    if (head[j]) grp[g] = make_int2((int)(keys[j] >> 32), r.ctg);
}

// per block: the number of its corners, and its key (haplotype * n_ctg + target) << 32 | start
__global__ __launch_bounds__(256) void hp_blocks(const cornetto_ivl_t *blocks, int64_t n, const int2 *grp, int32_t n_ctg, int32_t flank, uint32_t *cc, u64 *keys, uint32_t *vals)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const cornetto_ivl_t x = blocks[b];
    const int2 g = grp[x.ctg];
    cc[b] = (x.start >= flank ? 1u : 0u) + (x.finish >= flank ? 1u : 0u);                       // :58
    keys[b] = ((u64)((uint32_t)g.x * (uint32_t)n_ctg + (uint32_t)g.y) << 32) | (uint32_t)x.start;
    vals[b] = (uint32_t)b;
}

__device__ __forceinline__ int32_t hp_cap(long long v) { return (int32_t)(v < INT32_MAX ? v : INT32_MAX); }

__global__ __launch_bounds__(256) void hp_corners(const cornetto_ivl_t *blocks, int64_t n, const int2 *grp, int32_t flank, const uint32_t *off, cornetto_ivl_t *out)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const cornetto_ivl_t x = blocks[b];
    const int32_t ctg = grp[x.ctg].y;
    uint32_t o = off[b];
    if (x.start >= flank) out[o++] = cornetto_ivl_t{ctg, x.start - flank, hp_cap((long long)x.start + flank)};
    if (x.finish >= flank) out[o] = cornetto_ivl_t{ctg, x.finish - flank, hp_cap((long long)x.finish + flank)};
}

// the sorted blocks as intervals of their (haplotype, target) pair
__global__ __launch_bounds__(256) void hp_union_in(const cornetto_ivl_t *blocks, const u64 *keys, const uint32_t *vals, int64_t n, cornetto_ivl_t *out)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    out[j] = cornetto_ivl_t{(int32_t)(keys[j] >> 32), (int32_t)(uint32_t)keys[j], blocks[vals[j]].finish};
}

struct HpGapArgs {
    const cornetto_ivl_t *u;       // the merged blocks per (haplotype, target) pair p = haplotype * n_ctg + target, by (p, start)
    const u64 *n_u;                // their number (device)
    int64_t n_cap;                 // rows the grid covers (the number of blocks: at least *n_u)
    int64_t n_pair;                // n_hap * n_ctg
    const int32_t *ctg_len;
    int32_t n_ctg;
    uint32_t *has;                 // [n_pair] 1: the pair has a row (set by the counting pass, read by the pass over the pairs)
    uint32_t *cnt;                 // [n_cap + n_pair] gaps of row i / of pair p without rows
    const uint32_t *off;           // exclusive scan of cnt
    const u64 *base;               // the writing pass: where the gaps start in out (device: the number of corners)
    cornetto_ivl_t *out;
};

// the gaps row i of the merged list is responsible for: the one in front of it, and the one behind it when it is its pair's last row
__device__ __forceinline__ int hp_row_gaps(const HpGapArgs &A, int64_t i, int64_t n_u, cornetto_ivl_t (&g)[2], bool &first)
{
    const cornetto_ivl_t x = A.u[i];
    const int32_t ctg = x.ctg % A.n_ctg, len = A.ctg_len[ctg];
    first = i == 0 || A.u[i - 1].ctg != x.ctg;
    const int32_t prev_end = first ? 0 : A.u[i - 1].finish;
    const int32_t a = prev_end < len ? prev_end : len, b = x.start < len ? x.start : len;
    int k = 0;
    if (b > a) g[k++] = cornetto_ivl_t{ctg, a, b};
    const bool last = i == n_u - 1 || A.u[i + 1].ctg != x.ctg;
    if (last && x.finish < len) g[k++] = cornetto_ivl_t{ctg, x.finish, len};
    return k;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void hp_gap_rows(HpGapArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_cap) return;
    const int64_t n_u = (int64_t)*A.n_u;
    int k = 0;
    cornetto_ivl_t g[2];
    bool first = false;
    if (i < n_u) k = hp_row_gaps(A, i, n_u, g, first);
    if (!WRITE) {
        A.cnt[i] = (uint32_t)k;
        if (i < n_u && first) A.has[A.u[i].ctg] = 1u;
    } else {
        const u64 o = *A.base + A.off[i];
        for (int q = 0; q < k; ++q) A.out[o + q] = g[q];
    }
}

template <bool WRITE>
__global__ __launch_bounds__(256) void hp_gap_pairs(HpGapArgs A)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pair) return;
    const int32_t ctg = (int32_t)(p % A.n_ctg), len = A.ctg_len[ctg];
    const bool whole = !A.has[p] && len > 0;           // :55 a contig no block of the haplotype lies on
    if (!WRITE) A.cnt[A.n_cap + p] = whole ? 1u : 0u;
    else if (whole) A.out[*A.base + A.off[A.n_cap + p]] = cornetto_ivl_t{ctg, 0, len};
}

__global__ __launch_bounds__(256) void hp_key_ivl(const cornetto_ivl_t *v, int64_t n, u64 *keys, uint32_t *vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((u64)(uint32_t)v[i].ctg << 32) | (uint32_t)v[i].start;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void hp_gather(const cornetto_ivl_t *v, const uint32_t *vals, int64_t n, cornetto_ivl_t *out)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    out[j] = v[vals[j]];
}

int bits_for(int64_t n_values)     // bits that hold 0 .. n_values - 1
{
    int b = 0;
    while (b < 63 && ((int64_t)1 << b) < n_values) ++b;
    return b;
}

// a workspace block cut into 256-byte aligned pieces
struct Carve {
    uint8_t *p;
    size_t at = 0;
    explicit Carve(uint8_t *base) : p(base) {}
    template <class T>
    T *take(size_t n)
    {
        T *r = reinterpret_cast<T *>(p + at);
        at += (size_t)cn_align_up((int64_t)((n ? n : 1) * sizeof(T)), 256);
        return r;
    }
};

unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

int hap_fun_stage(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_hap_row_t *rows, const int64_t *n_rows, int32_t n_hap, int64_t N,
                  const cornetto_hap_opt_t *opt, cornetto_ivl_t **fun, int64_t *n_fun)
{
    const int64_t P = (int64_t)n_hap * n_ctg;
    const int pos_bits = 32 + bits_for(n_ctg), hap_bits = 32 + bits_for(n_hap), pair_bits = 32 + bits_for(P);
    u64 *p_cnt = (u64 *)cn_pin(h, PIN_SMALL, 64);
    if (!p_cnt) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");

    // ---- the rows -> blocks (:48-51) ----
    size_t need = 0;
    {
        Carve c(nullptr);
        c.take<u64>(8); c.take<int32_t>((size_t)n_ctg); c.take<int64_t>((size_t)n_hap + 1); c.take<cornetto_hap_row_t>((size_t)N); c.take<u64>((size_t)N);
        c.take<uint32_t>((size_t)N); c.take<uint32_t>((size_t)N); c.take<uint32_t>((size_t)N); c.take<cornetto_ivl_t>((size_t)N); c.take<cornetto_ivl_t>((size_t)N);
        c.take<int2>((size_t)N); c.take<uint8_t>(cnivl::ws_bytes((size_t)N));
        need = c.at;
    }
    uint8_t *wa = (uint8_t *)cn_ws(h, WS_HAP_ROWS, need);
    if (!wa) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");
    Carve ca(wa);
    u64 *d_cnt = ca.take<u64>(8);                      // [0] blocks, [1] corners, [2] merged blocks per pair, [3] gaps, [4] funbits
    int32_t *d_len = ca.take<int32_t>((size_t)n_ctg);
    int64_t *d_pref = ca.take<int64_t>((size_t)n_hap + 1);
    cornetto_hap_row_t *d_rows = ca.take<cornetto_hap_row_t>((size_t)N);
    u64 *d_keys = ca.take<u64>((size_t)N);
    uint32_t *d_vals = ca.take<uint32_t>((size_t)N), *d_head = ca.take<uint32_t>((size_t)N), *d_rank = ca.take<uint32_t>((size_t)N);
    cornetto_ivl_t *d_ivl = ca.take<cornetto_ivl_t>((size_t)N), *d_blocks = ca.take<cornetto_ivl_t>((size_t)N);
    int2 *d_grp = ca.take<int2>((size_t)N);
    uint8_t *d_mws = ca.take<uint8_t>(cnivl::ws_bytes((size_t)N));
    std::vector<int64_t> pref((size_t)n_hap + 1, 0);
    for (int32_t k = 0; k < n_hap; ++k) pref[(size_t)k + 1] = pref[(size_t)k] + n_rows[k];
    CN_HIP(h, hipMemsetAsync(d_cnt, 0, 64, h->stream));
    if (n_ctg > 0) CN_HIP(h, hipMemcpyAsync(d_len, ctg_len, (size_t)n_ctg * 4, hipMemcpyHostToDevice, h->stream));
    CN_HIP(h, hipMemcpyAsync(d_pref, pref.data(), pref.size() * 8, hipMemcpyHostToDevice, h->stream));
    int64_t B = 0;
    if (N > 0) {
        CN_HIP(h, hipMemcpyAsync(d_rows, rows, (size_t)N * sizeof(cornetto_hap_row_t), hipMemcpyHostToDevice, h->stream));
        uint8_t *sws = (uint8_t *)cn_ws(h, WS_SORT, cnsort::ws_bytes(N));
        if (!sws) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");
        u64 *rk = nullptr;
        uint32_t *rv = nullptr;
        CN_LAUNCH(h, "hp_key_pos", hp_key_pos<<<dim3(grid256(N)), dim3(256), 0, h->stream>>>(d_rows, N, d_keys, d_vals));
        CN_TRY(cnsort::pairs_u64(h, "hp_sort_pos", d_keys, d_vals, N, sws, pos_bits, &rk, &rv));
        CN_LAUNCH(h, "hp_key_query", hp_key_query<<<dim3(grid256(N)), dim3(256), 0, h->stream>>>(d_rows, rv, N, d_pref, n_hap, d_keys, d_vals));
        CN_TRY(cnsort::pairs_u64(h, "hp_sort_query", d_keys, d_vals, N, sws, hap_bits, &rk, &rv));
        CN_LAUNCH(h, "hp_heads", hp_heads<<<dim3(grid256(N)), dim3(256), 0, h->stream>>>(d_rows, rk, rv, N, d_head));
        CN_TRY(cnscan::exclusive_u32(h, "hp_group_scan", d_head, N, 1, d_rank, nullptr));
        CN_LAUNCH(h, "hp_groups", hp_groups<<<dim3(grid256(N)), dim3(256), 0, h->stream>>>(d_rows, rk, rv, N, d_head, d_rank, d_ivl, d_grp));
        CN_TRY(cnivl::merge(h, "hp_block_merge", d_ivl, N, opt->merge_dist, d_mws, d_blocks, d_cnt));
        CN_HIP(h, hipMemcpyAsync(p_cnt, d_cnt, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        B = (int64_t)p_cnt[0];
        if (B < 1 || B > N) return cn_fail(h, CORNETTO_E_HIP, "hap_fun: %lld blocks of %lld rows", (long long)B, (long long)N);
    } else {
        CN_HIP(h, hipStreamSynchronize(h->stream));   // (`pref` is pageable memory of this frame)
    }

    // ---- blocks -> corners (:58) and gaps (:55) ----
    const int64_t m_cap = 4 * B + P;                   // corners: 2 per block; gaps: one in front of every merged block, one behind a pair's last, one per empty pair
    {
        Carve c(nullptr);
        c.take<uint32_t>((size_t)B); c.take<uint32_t>((size_t)B); c.take<u64>((size_t)B); c.take<uint32_t>((size_t)B); c.take<cornetto_ivl_t>((size_t)B);
        c.take<cornetto_ivl_t>((size_t)B); c.take<uint8_t>(cnivl::ws_bytes((size_t)B)); c.take<uint32_t>((size_t)(B + P)); c.take<uint32_t>((size_t)(B + P));
        c.take<uint32_t>((size_t)P); c.take<cornetto_ivl_t>((size_t)m_cap);
        need = c.at;
    }
    uint8_t *wb = (uint8_t *)cn_ws(h, WS_HAP_BLOCKS, need);
    if (!wb) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");
    Carve cb(wb);
    uint32_t *d_cc = cb.take<uint32_t>((size_t)B), *d_coff = cb.take<uint32_t>((size_t)B);
    u64 *d_bkeys = cb.take<u64>((size_t)B);
    uint32_t *d_bvals = cb.take<uint32_t>((size_t)B);
    cornetto_ivl_t *d_uin = cb.take<cornetto_ivl_t>((size_t)B), *d_u = cb.take<cornetto_ivl_t>((size_t)B);
    uint8_t *d_mws2 = cb.take<uint8_t>(cnivl::ws_bytes((size_t)B));
    uint32_t *d_gcnt = cb.take<uint32_t>((size_t)(B + P)), *d_goff = cb.take<uint32_t>((size_t)(B + P)), *d_has = cb.take<uint32_t>((size_t)P);
    cornetto_ivl_t *d_parts = cb.take<cornetto_ivl_t>((size_t)m_cap);
    if (B > 0) {
        uint8_t *sws = (uint8_t *)cn_ws(h, WS_SORT, cnsort::ws_bytes(B));
        if (!sws) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");
        u64 *rk = nullptr;
        uint32_t *rv = nullptr;
        CN_LAUNCH(h, "hp_blocks", hp_blocks<<<dim3(grid256(B)), dim3(256), 0, h->stream>>>(d_blocks, B, d_grp, n_ctg, opt->flank, d_cc, d_bkeys, d_bvals));
        CN_TRY(cnscan::exclusive_u32(h, "hp_corner_scan", d_cc, B, 1, d_coff, d_cnt + 1));
        CN_LAUNCH(h, "hp_corners", hp_corners<<<dim3(grid256(B)), dim3(256), 0, h->stream>>>(d_blocks, B, d_grp, opt->flank, d_coff, d_parts));
        CN_TRY(cnsort::pairs_u64(h, "hp_sort_blocks", d_bkeys, d_bvals, B, sws, pair_bits, &rk, &rv));
        CN_LAUNCH(h, "hp_union_in", hp_union_in<<<dim3(grid256(B)), dim3(256), 0, h->stream>>>(d_blocks, rk, rv, B, d_uin));
        CN_TRY(cnivl::merge(h, "hp_union_merge", d_uin, B, 0, d_mws2, d_u, d_cnt + 2));
    }
    int64_t M = 0;
    if (B + P > 0) {
        HpGapArgs G{d_u, d_cnt + 2, B, P, d_len, n_ctg, d_has, d_gcnt, d_goff, d_cnt + 1, d_parts};
        if (P > 0) CN_HIP(h, hipMemsetAsync(d_has, 0, (size_t)P * 4, h->stream));
        if (B > 0) CN_LAUNCH(h, "hp_gap_count", hp_gap_rows<false><<<dim3(grid256(B)), dim3(256), 0, h->stream>>>(G));
        if (P > 0) CN_LAUNCH(h, "hp_gap_count", hp_gap_pairs<false><<<dim3(grid256(P)), dim3(256), 0, h->stream>>>(G));
        CN_TRY(cnscan::exclusive_u32(h, "hp_gap_scan", d_gcnt, B + P, 1, d_goff, d_cnt + 3));
        if (B > 0) CN_LAUNCH(h, "hp_gap_write", hp_gap_rows<true><<<dim3(grid256(B)), dim3(256), 0, h->stream>>>(G));
        if (P > 0) CN_LAUNCH(h, "hp_gap_write", hp_gap_pairs<true><<<dim3(grid256(P)), dim3(256), 0, h->stream>>>(G));
        CN_HIP(h, hipMemcpyAsync(p_cnt, d_cnt, 32, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        M = (int64_t)(p_cnt[1] + p_cnt[3]);
        if (p_cnt[1] > (u64)(2 * B) || p_cnt[3] > (u64)(2 * B + P)) return cn_fail(h, CORNETTO_E_HIP, "hap_fun: %llu corners and %llu gaps of %lld blocks", p_cnt[1], p_cnt[3], (long long)B);
    }

    // ---- gaps + corners -> funbits (:61, :67) ----
    cornetto_ivl_t *o = nullptr;
    int64_t m = 0;
    if (M > 0) {
        {
            Carve c(nullptr);
            c.take<u64>((size_t)M); c.take<uint32_t>((size_t)M); c.take<cornetto_ivl_t>((size_t)M); c.take<cornetto_ivl_t>((size_t)M); c.take<uint8_t>(cnivl::ws_bytes((size_t)M));
            need = c.at;
        }
        uint8_t *wc = (uint8_t *)cn_ws(h, WS_HAP_FUN, need);
        uint8_t *sws = (uint8_t *)cn_ws(h, WS_SORT, cnsort::ws_bytes(M));
        if (!wc || !sws) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: workspace allocation failed");
        Carve cc(wc);
        u64 *d_fkeys = cc.take<u64>((size_t)M);
        uint32_t *d_fvals = cc.take<uint32_t>((size_t)M);
        cornetto_ivl_t *d_sorted = cc.take<cornetto_ivl_t>((size_t)M), *d_out = cc.take<cornetto_ivl_t>((size_t)M);
        uint8_t *d_mws3 = cc.take<uint8_t>(cnivl::ws_bytes((size_t)M));
        u64 *rk = nullptr;
        uint32_t *rv = nullptr;
        CN_LAUNCH(h, "hp_key_fun", hp_key_ivl<<<dim3(grid256(M)), dim3(256), 0, h->stream>>>(d_parts, M, d_fkeys, d_fvals));
        CN_TRY(cnsort::pairs_u64(h, "hp_sort_fun", d_fkeys, d_fvals, M, sws, pos_bits, &rk, &rv));
        CN_LAUNCH(h, "hp_gather", hp_gather<<<dim3(grid256(M)), dim3(256), 0, h->stream>>>(d_parts, rv, M, d_sorted));
        CN_TRY(cnivl::merge(h, "hp_fun_merge", d_sorted, M, 0, d_mws3, d_out, d_cnt + 4));
        CN_HIP(h, hipMemcpyAsync(p_cnt, d_cnt + 4, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        m = (int64_t)p_cnt[0];
        if (m < 1 || m > M) return cn_fail(h, CORNETTO_E_HIP, "hap_fun: %lld funbits of %lld parts", (long long)m, (long long)M);
        o = (cornetto_ivl_t *)cn_result_alloc((size_t)m * sizeof(cornetto_ivl_t));
        if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: host allocation failed");
        if (hipMemcpyAsync(o, d_out, (size_t)m * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
            cornetto_free(o);
            return cn_fail(h, CORNETTO_E_HIP, "hap_fun: copy back failed");
        }
    }
    if (!o) {
        o = (cornetto_ivl_t *)malloc(sizeof(cornetto_ivl_t));
        if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "hap_fun: host allocation failed");
    }
    *fun = o;
    *n_fun = m;
    return CORNETTO_OK;
}

}  // namespace

extern "C" {

void cornetto_hap_defaults(cornetto_hap_opt_t *o)
{
    if (!o) return;
    o->merge_dist = 1000000;    /* create-hapnetto.sh:50 */
    o->flank = 500;             /* :58 */
}

int cornetto_hap_fun(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_hap_row_t *rows, const int64_t *n_rows, int32_t n_hap,
                     const cornetto_hap_opt_t *opt, cornetto_ivl_t **fun, int64_t *n_fun)
{
    if (!h || !fun || !n_fun || !opt || n_ctg < 0 || n_hap < 0 || (n_ctg > 0 && !ctg_len) || (n_hap > 0 && !n_rows) || opt->merge_dist < 0 || opt->flank < 1)
        return cn_fail(h, CORNETTO_E_ARG, "hap_fun: bad argument");
    *fun = nullptr;
    *n_fun = 0;
    int64_t N = 0;
    for (int32_t k = 0; k < n_hap; ++k) {
        if (n_rows[k] < 0) return cn_fail(h, CORNETTO_E_ARG, "hap_fun: haplotype %d has a negative row count", k);
        N += n_rows[k];
        if (N > ((int64_t)1 << 28)) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "hap_fun: more than 2^28 rows");
    }
    if (N > 0 && !rows) return cn_fail(h, CORNETTO_E_ARG, "hap_fun: bad argument");
    if ((int64_t)n_hap * n_ctg > 0x7FFFFFFFll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "hap_fun: %d haplotypes x %d contigs", n_hap, n_ctg);
    for (int32_t c = 0; c < n_ctg; ++c)
        if (ctg_len[c] < 0) return cn_fail(h, CORNETTO_E_ARG, "hap_fun: contig %d has a negative length", c);
    for (int64_t i = 0; i < N; ++i)
        if (rows[i].ctg < 0 || rows[i].ctg >= n_ctg || rows[i].start < 0 || rows[i].finish <= rows[i].start)
            return cn_fail(h, CORNETTO_E_ARG, "hap_fun: row %lld (target %d, %d to %d) is not an interval on a contig of the assembly", (long long)i, rows[i].ctg,
                           rows[i].start, rows[i].finish);
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int rc = hap_fun_stage(h, ctg_len, n_ctg, rows, n_rows, n_hap, N, opt, fun, n_fun);
    cn_timing_end(h);
    return rc;
}

}  // extern "C"
