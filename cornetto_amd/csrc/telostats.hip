// telostats.hip — cornetto_telo_ends(): the telomere regions at the contig ends of scripts/telostats.sh:35-47 for gfx950, from the mark
// bitmap of the telomere scan (telo.hip) to the rows of PREFIX.windows.0.4.50kb.ends.bed without a window list, an atomic, a sort or a
// text file in between:
//     telofind | awk | telowin 99.9 0.4 | awk | bedtools merge -d 100 | bedtools intersect -wa -b <contig ends>
//
// The qualifying windows of one contig are window indices j (start 200 j, end min(200 j + 1000, L)); only the last visited window is
// clipped, so the ends are non-decreasing in j and `bedtools merge -d d` is a run-length rule on one bit q[j] per window: with
// G = (1000 + d) / 200, consecutive qualifying windows j < j' lie in one region iff 200 j' <= 200 j + 1000 + d, i.e. j' - j <= G (the
// clipped window is the last one: nothing starts behind it).  So
//     head[j] = q[j] and no q in [j - G, j - 1]        tail[j] = q[j] and no q in [j + 1, j + G]
// and the r-th head of the assembly pairs with its r-th tail (a look never crosses a contig, every region has one of each).  G <= 63:
// a look fits the neighbouring 64-bit word.
//
// te_qual   telowin's window counts (telowin_tile.hpp, as tw_scan) -> q: each wave ballots its 64 windows, four words per tile of 256
//           windows; tiles never share a word, plain stores.
// te_runs   one thread per word: heads and tails from the word and its two neighbours in the same contig, their counts.
//           The counts go through the device scan (scan.hpp): every word's place in the region list.
// te_place  region starts by head rank, region ends by tail rank.
// te_ends   k = end intervals a region overlaps ([0, E) and [L - E, L) if L > 2 E, else [0, L): scripts/telostats.sh:44), scanned;
// te_emit   every region k times (bedtools intersect -wa prints A once per overlapping B), in region order.
// The region list is sized by what the last call on the handle needed; the counted total is checked and the placement rerun with the
// true size when it did not fit (never a truncated answer).
#include "common.hpp"
#include "scan.hpp"
#include "telowin_tile.hpp"
#include "internal.hpp"

namespace {

struct TeQualArgs {
    const unsigned long long *bitmap;
    const int64_t *bit_off;   // [n_ctg] first bit of contig (multiple of 64)
    const int32_t *ctg_len;
    const int2 *tiles;        // {ctg, first window index}
    double thr;
    unsigned long long *flags;   // [4 n_tiles]: bit b of word 4 t + w = window tiles[t].y + 64 w + b qualifies
};

__global__ __launch_bounds__(256) void te_qual(TeQualArgs A)
{
    __shared__ int bc[cntw::TW_BLOCKS];
    __shared__ unsigned long long sw[cntw::TW_WORDS];
    const int2 tile = A.tiles[blockIdx.x];
    const cntw::Window w = cntw::tile_window(A.bitmap, A.bit_off[tile.x], A.ctg_len[tile.x], tile, bc, sw);
    const int den = w.end - w.start;
    const bool q = w.visited && den > 0 && (double)w.car / den >= A.thr;      // src/telomere_windows.c:36-37
    const unsigned long long b = __builtin_amdgcn_ballot_w64(q);
    if ((threadIdx.x & 63) == 0) A.flags[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = b;
}

// bit j of the result: a set bit of (lo:hi) in [j - k, j - 1], for the 64 positions of hi (bit i of lo = position i - 64); 1 <= k <= 63.
// The pair is moved up by one, then the covered width doubles per step (1, 2, 4, ... then the rest).
__device__ __forceinline__ unsigned long long reach_back(unsigned long long hi, unsigned long long lo, int k)
{
    hi = (hi << 1) | (lo >> 63);
    lo <<= 1;
    int w = 1;                                          // every set bit p covers [p, p + w) so far
    while (w < k) {
        const int s = w < k - w ? w : k - w;            // s <= 32
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        w += s;
    }
    return hi;
}

struct TeRunArgs {
    const unsigned long long *flags;
    const int2 *tiles;
    int64_t n_tiles;
    int32_t G;
    unsigned long long *heads, *tails;   // [4 n_tiles]
    uint2 *cnt;                          // [4 n_tiles] {heads, tails} of the word
};

__global__ __launch_bounds__(256) void te_runs(TeRunArgs A)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 4 * A.n_tiles) return;
    const unsigned long long cur = A.flags[w];
    unsigned long long hd = 0, tl = 0;
    if (cur) {
        // the windows of a contig are consecutive bits of consecutive words (a tile that is not the contig's last holds 256 of them): the
        // word in front and the word behind, unless it belongs to another contig
        const int64_t t = w >> 2;
        const int k = (int)(w & 3), ctg = A.tiles[t].x;
        const unsigned long long prev = (k > 0 || (t > 0 && A.tiles[t - 1].x == ctg)) ? A.flags[w - 1] : 0ull;
        const unsigned long long next = (k < 3 || (t + 1 < A.n_tiles && A.tiles[t + 1].x == ctg)) ? A.flags[w + 1] : 0ull;
        hd = cur & ~reach_back(cur, prev, A.G);
        tl = cur & ~__brevll(reach_back(__brevll(cur), __brevll(next), A.G));      // (the same looking ahead: positions mirrored)
    }
    A.heads[w] = hd;
    A.tails[w] = tl;
    A.cnt[w] = make_uint2((unsigned)__popcll(hd), (unsigned)__popcll(tl));
}

struct TePlaceArgs {
    const unsigned long long *heads, *tails;
    const uint32_t *off_h, *off_t;       // exclusive scans of cnt
    const int2 *tiles;
    const int32_t *ctg_len;
    int64_t n_tiles;
    uint32_t cap;
    int2 *rs;                            // [cap] {ctg, start}
    int32_t *re;                         // [cap] end
};

__global__ __launch_bounds__(256) void te_place(TePlaceArgs A)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 4 * A.n_tiles) return;
    unsigned long long hd = A.heads[w], tl = A.tails[w];
    if (!(hd | tl)) return;
    const int2 tile = A.tiles[w >> 2];
    const int j0 = tile.y + 64 * (int)(w & 3);
    uint32_t ih = A.off_h[w], it = A.off_t[w];
    while (hd) {
        const int b = __ffsll((long long)hd) - 1;
        hd &= hd - 1;
        if (ih < A.cap) A.rs[ih] = make_int2(tile.x, (j0 + b) * 200);
        ++ih;
    }
    if (tl) {
        const long long len = A.ctg_len[tile.x];
        while (tl) {
            const int b = __ffsll((long long)tl) - 1;
            tl &= tl - 1;
            const long long e = (long long)(j0 + b) * 200 + 1000;
            if (it < A.cap) A.re[it] = (int32_t)(e < len ? e : len);
            ++it;
        }
    }
}

struct TeEndArgs {
    const int2 *rs;
    const int32_t *re;
    const int32_t *ctg_len;
    const unsigned long long *tot;       // [0] regions (heads), [1] tails
    uint32_t cap;
    int32_t ends;
    uint32_t *kk;                        // [cap] copies of region i (0 behind the last region)
    const uint32_t *off_k;               // te_emit: exclusive scan of kk
    cornetto_ivl_t *rows;                // te_emit: [2 cap]
};

__global__ __launch_bounds__(256) void te_ends(TeEndArgs A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.cap) return;
    uint32_t k = 0;
    if ((unsigned long long)i < A.tot[0]) {
        const int2 r = A.rs[i];
        const long long s = r.y, e = A.re[i], L = A.ctg_len[r.x], E = A.ends;
        k = L > 2 * E ? (uint32_t)(s < E) + (uint32_t)(e > L - E) : 1u;            // (a region is not empty and lies in [0, L))
    }
    A.kk[i] = k;
}

__global__ __launch_bounds__(256) void te_emit(TeEndArgs A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.cap || (unsigned long long)i >= A.tot[0]) return;
    const uint32_t k = A.kk[i], o = A.off_k[i];
    if (!k) return;
    const int2 r = A.rs[i];
    const cornetto_ivl_t v{r.x, r.y, A.re[i]};
    A.rows[o] = v;                       // (o + k <= 2 cap: k <= 2 for each of at most cap regions)
    if (k > 1) A.rows[o + 1] = v;
}

// the regions at the contig ends from the marks `d_marks` in the window layout of `a`
int telo_ends_stage(cornetto_accel_t *h, const cornetto_asm_t *a, const unsigned long long *d_marks, double thr, int32_t G, int32_t ends, cornetto_ivl_t **rows,
                    int64_t *n_rows)
{
    const size_t nt = (size_t)a->tw_n_tiles, nw = 4 * nt;
    cornetto_ivl_t *out = nullptr;
    size_t n_out = 0;
    if (nt > 0) {
        if (nw > 0x7fffffffull) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "telo_ends: too many window tiles");
        uint8_t *ws = (uint8_t *)cn_ws(h, WS_TE_WORDS, nw * (3 * 8 + sizeof(uint2) + 2 * 4) + 4 * 4);
        unsigned long long *d_tot = (unsigned long long *)cn_ws(h, WS_TE_CNT, 64);
        unsigned long long *p_tot = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
        if (!ws || !d_tot || !p_tot) return cn_fail(h, CORNETTO_E_NOMEM, "telo_ends: workspace allocation failed");
        unsigned long long *d_flags = reinterpret_cast<unsigned long long *>(ws), *d_heads = d_flags + nw, *d_tails = d_heads + nw;
        uint2 *d_cnt = reinterpret_cast<uint2 *>(d_tails + nw);
        uint32_t *d_off[2] = {reinterpret_cast<uint32_t *>(d_cnt + nw), reinterpret_cast<uint32_t *>(d_cnt + nw) + nw};
        CN_HIP(h, hipMemsetAsync(d_tot, 0, 64, h->stream));
        TeQualArgs Q{d_marks, a->d_tw_boff, a->d_len, a->d_tw_tiles, thr, d_flags};
        CN_LAUNCH(h, "te_qual", te_qual<<<dim3((unsigned)nt), dim3(256), 0, h->stream>>>(Q));
        TeRunArgs R{d_flags, a->d_tw_tiles, (int64_t)nt, G, d_heads, d_tails, d_cnt};
        CN_LAUNCH(h, "te_runs", te_runs<<<dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream>>>(R));
        CN_TRY(cnscan::exclusive_u32_multi(h, "te_order", reinterpret_cast<const uint32_t *>(d_cnt), (int64_t)nw, 2, 2, d_off, d_tot));
        // the region list: room for what the last call on this handle needed
        size_t cap = std::max<size_t>(4096, h->te_cap);
        const int force = CN_DEV_INT("CORNETTO_TE_CAP_FORCE", 0);   // (tests: an estimate that does not hold)
        if (force > 0) cap = (size_t)force;
        for (int attempt = 0; attempt < 2; ++attempt) {
            uint8_t *wr = (uint8_t *)cn_ws(h, WS_TE_REG, cap * (sizeof(int2) + 3 * 4) + 4 * 4);
            cornetto_ivl_t *d_rows = (cornetto_ivl_t *)cn_ws(h, WS_TE_ROWS, 2 * cap * sizeof(cornetto_ivl_t));
            const size_t spec = std::min<size_t>(2 * cap, 8192);    // the count and, with it, the first rows (an assembly has a few hundred): one round trip
            cornetto_ivl_t *p_rows = (cornetto_ivl_t *)cn_pin(h, PIN_TE, spec * sizeof(cornetto_ivl_t));
            if (!wr || !d_rows || !p_rows) return cn_fail(h, CORNETTO_E_NOMEM, "telo_ends: workspace allocation failed");
            int2 *d_rs = reinterpret_cast<int2 *>(wr);
            int32_t *d_re = reinterpret_cast<int32_t *>(d_rs + cap);
            uint32_t *d_kk = reinterpret_cast<uint32_t *>(d_re + cap), *d_offk = d_kk + cap;
            TePlaceArgs P{d_heads, d_tails, d_off[0], d_off[1], a->d_tw_tiles, a->d_len, (int64_t)nt, (uint32_t)cap, d_rs, d_re};
            CN_LAUNCH(h, "te_place", te_place<<<dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream>>>(P));
            TeEndArgs E{d_rs, d_re, a->d_len, d_tot, (uint32_t)cap, ends, d_kk, d_offk, d_rows};
            const unsigned nb = (unsigned)((cap + 255) / 256);
            CN_LAUNCH(h, "te_ends", te_ends<<<dim3(nb), dim3(256), 0, h->stream>>>(E));
            CN_TRY(cnscan::exclusive_u32(h, "te_order", d_kk, (int64_t)cap, 1, d_offk, d_tot + 2));
            CN_LAUNCH(h, "te_emit", te_emit<<<dim3(nb), dim3(256), 0, h->stream>>>(E));
            CN_HIP(h, hipMemcpyAsync(p_tot, d_tot, 32, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipMemcpyAsync(p_rows, d_rows, spec * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            const unsigned long long n_reg = p_tot[0], n_row = p_tot[2];
            if (p_tot[1] != n_reg) return cn_fail(h, CORNETTO_E_HIP, "telo_ends: %llu region starts and %llu region ends", n_reg, p_tot[1]);
            if (n_reg > 0x7fffffffull) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "telo_ends: %llu regions", n_reg);
            if (n_reg > cap) {                                      // exact retry with the true size; never a truncated answer
                if (attempt == 1) return cn_fail(h, CORNETTO_E_HIP, "telo_ends: %llu regions after resizing", n_reg);
                cap = (size_t)n_reg;
                continue;
            }
            if (n_row > 2 * n_reg) return cn_fail(h, CORNETTO_E_HIP, "telo_ends: %llu rows of %llu regions", n_row, n_reg);
            if (force <= 0) h->te_cap = std::max<size_t>(h->te_cap, (size_t)n_reg + (size_t)n_reg / 8);
            n_out = (size_t)n_row;
            out = (cornetto_ivl_t *)malloc((n_out ? n_out : 1) * sizeof(cornetto_ivl_t));
            if (!out) return cn_fail(h, CORNETTO_E_NOMEM, "telo_ends: host allocation failed");
            if (n_out) memcpy(out, p_rows, std::min(n_out, spec) * sizeof(cornetto_ivl_t));
            if (n_out > spec) {
                const hipError_t e = hipMemcpy(out + spec, d_rows + spec, (n_out - spec) * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost);
                if (e != hipSuccess) {
                    free(out);
                    return cn_fail(h, CORNETTO_E_HIP, "telo_ends: copying the rows -> %s", hipGetErrorString(e));
                }
            }
            break;
        }
    }
    if (!out) {
        out = (cornetto_ivl_t *)malloc(sizeof(cornetto_ivl_t));
        if (!out) return cn_fail(h, CORNETTO_E_NOMEM, "telo_ends: host allocation failed");
    }
    *rows = out;
    *n_rows = (int64_t)n_out;
    return CORNETTO_OK;
}

}  // namespace

extern "C" int cornetto_telo_ends(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, double thr_adj, int32_t merge_dist, int32_t ends,
                                  cornetto_ivl_t **rows, int64_t *n_rows)
{
    if (!h || !a || !motif || !rows || !n_rows || ends < 1) return cn_fail(h, CORNETTO_E_ARG, "telo_ends: bad argument");
    *rows = nullptr;
    *n_rows = 0;
    if (merge_dist < 0 || merge_dist > CORNETTO_TELO_ENDS_MAX_DIST)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, "telo_ends: merge distance %d; 0 to %d are supported", merge_dist, CORNETTO_TELO_ENDS_MAX_DIST);
    const int32_t G = (1000 + merge_dist) / 200;      // <= 63: a look-back fits one 64-bit word
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const unsigned long long *d_marks = nullptr;
    int rc = cn_telo_marks_impl(h, a, motif, &d_marks);
    if (rc == CORNETTO_OK) rc = telo_ends_stage(h, a, d_marks, thr_adj, G, ends, rows, n_rows);
    cn_timing_end(h);
    return rc;
}
