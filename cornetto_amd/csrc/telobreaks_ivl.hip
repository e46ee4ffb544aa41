// telobreaks_ivl.hip — the telomere breaks as a rule on intervals, for gfx950: cornetto_telo_breaks() (a resident assembly: sdust and
// telofind run here and neither list leaves the device) and cornetto_telobreaks_ivl() (explicit lists).  Replaces the chain of
// test/realtest.sh:65-69 of the reference,
//     cornetto sdust asm.fa > asm.sdust;  cornetto telofind asm.fa > asm.telomere;  cornetto telobreaks asm.lens asm.sdust asm.telomere
// with src/telomere_breaks.c:79-148 behind it, for lists that sdust itself made.
//
// The reference keeps one bit per base (telobreaks.hip does the same, 64 bits per word).  What sdust prints needs no bitset: its
// save_masked_regions (src/sdust/sdust.c:88-102) merges an interval that starts at or before the previous finish, so inside one contig
// the list is sorted and every start lies beyond the previous finish — the intervals ARE the runs of the bitset, one clear bit at least
// between two of them.  Then :95-148 says:
//     a row with matched >= 24 (:98) and flanks a = max(0, start - 100), b = min(L, end + 100) (:102-103) marks the one interval
//     [s, min(f, L)) with s <= a and min(f, L) >= b: only the last interval that starts at or before a can hold a, and all of [a, b) is
//     set iff that one reaches b; the run around [start, end) (:114-121) is that interval;
//     every marked interval prints once as max(s - 1, 0) to min(f, L) - 1 (:139-142).
//   bk_check  one thread per interval: the precondition (order, a gap of one base at least, a contig of the table), the flag cleared
//   bk_mark   one thread per row: one binary search over the whole list on the key contig << 32 | start, a plain store of 1 into the
//             interval's flag (every writer stores the same value)
//             the flags go through the device scan (scan.hpp): every marked interval's rank
//   bk_emit   one thread per interval: a marked one writes its record at its rank — by contig, then by start, as tb_emit orders them
// O(intervals + rows log intervals) words instead of 2 x bases / 64; the count comes back with one 8-byte copy, then exactly n records.
#include "common.hpp"
#include "internal.hpp"
#include "scan.hpp"

namespace {

using u64 = unsigned long long;

constexpr int BK_MIN_TEL = 24;          // MIN_TEL, src/telomere_breaks.c:10
constexpr int BK_FLANK = 100;           // :102-103
constexpr uint32_t BK_E_IVL = 1u, BK_E_ROW = 2u, BK_E_ORDER = 4u;   // the error word (1 and 2 as tb_fill / tb_mark set them)

struct BkArgs {
    const int32_t *ctg_len;
    int32_t n_ctg;
    const cornetto_ivl_t *sd;           // by (ctg, start), disjoint and not touching inside a contig (bk_check)
    int64_t n_sd;
    uint32_t *flag;                     // [n_sd] 1 = the interval holds a row with its flanks
    const uint32_t *rank;               // [n_sd] exclusive scan of flag
    u64 *tot;                           // the scan's total; bk_emit puts the error word into its upper half
    uint32_t *err;
    cornetto_ivl_t *out;                // [n_sd]
};

__device__ __forceinline__ u64 bk_key(int32_t ctg, int32_t start) { return ((u64)(uint32_t)ctg << 32) | (uint32_t)start; }

__global__ __launch_bounds__(256) void bk_check(BkArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_sd) return;
    A.flag[i] = 0;
    const cornetto_ivl_t v = A.sd[i];
    if (v.ctg < 0 || v.ctg >= A.n_ctg) { atomicOr(A.err, BK_E_ORDER); return; }
    if (v.start < 0) { atomicOr(A.err, BK_E_IVL); return; }                      // (as tb_fill: no reading in the reference)
    if (i == 0) return;
    const cornetto_ivl_t p = A.sd[i - 1];
    if (p.ctg > v.ctg || (p.ctg == v.ctg && (v.start <= p.finish || v.start <= p.start))) atomicOr(A.err, BK_E_ORDER);
}

// rows: cornetto_telrow_t {ctg, start, end, matched}, or — hits != 0 — cornetto_hit_t {ctg, strand, start, end}, whose matched length is
// end - start (the sixth column `cornetto telofind` prints)
__global__ __launch_bounds__(256) void bk_mark(BkArgs A, const int4 *rows, int64_t n, int hits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 r = rows[i];
    const int32_t ctg = r.x, start = hits ? r.z : r.y, end = hits ? r.w : r.z;
    const long long matched = hits ? (long long)end - start : r.w;
    if (matched < BK_MIN_TEL) return;                                            // :98
    if (ctg < 0 || ctg >= A.n_ctg) return;                                       // :100
    const int32_t len = A.ctg_len[ctg];
    if (start < 0 || end > len || start >= end) { atomicOr(A.err, BK_E_ROW); return; }
    const int32_t a = start - BK_FLANK < 0 ? 0 : start - BK_FLANK;               // :102
    const int32_t b = (long long)end + BK_FLANK > len ? len : end + BK_FLANK;    // :103
    const u64 key = bk_key(ctg, a);
    int64_t lo = 0, hi = A.n_sd;                                                 // lo = intervals whose key is <= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const cornetto_ivl_t m = A.sd[mid];
        if (bk_key(m.ctg, m.start) <= key) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return;                                                         // in front of the first interval
    const cornetto_ivl_t v = A.sd[lo - 1];
    if (v.ctg != ctg) return;                                                    // the last interval of an earlier contig: not a neighbour
    if ((v.finish > len ? len : v.finish) >= b) A.flag[lo - 1] = 1u;
}

__global__ __launch_bounds__(256) void bk_emit(BkArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_sd) return;
    if (i == 0) *A.tot |= (u64)*A.err << 32;                                     // (the total is below 2^31: one word tells the host both)
    if (!A.flag[i]) return;
    const cornetto_ivl_t v = A.sd[i];
    const int32_t len = A.ctg_len[v.ctg];                                        // (a flagged interval passed bk_check's contig test)
    A.out[A.rank[i]] = cornetto_ivl_t{v.ctg, v.start - 1 < 0 ? 0 : v.start - 1, (v.finish > len ? len : v.finish) - 1};   // :139-142
}

// The rule over lists that are on the device.  `bad_list`: the status of a list that fails bk_check — the caller's mistake for an
// explicit list, a broken invariant for one sdust.hip made.  Synchronises.  (The workspaces are those of cornetto_telobreaks(): a handle
// runs one call at a time.)
int bk_stage(cornetto_accel_t *h, const char *who, const int32_t *d_len, int32_t n_ctg, const cornetto_ivl_t *d_sd, int64_t n_sd, const void *d_rows, int64_t n_rows,
             int hits, int bad_list, cornetto_ivl_t **out, int64_t *n_out)
{
    cornetto_ivl_t *o = nullptr;
    int64_t n = 0;
    if (n_sd > 0x7fffffffll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "%s: %lld low-complexity intervals, at most 2^31-1 are supported", who, (long long)n_sd);
    if (n_sd > 0) {
        // flags | ranks ; records out ; total (+ error word in its upper half), error word
        uint32_t *d_flag = (uint32_t *)cn_ws(h, WS_TB_OUT, (size_t)n_sd * (2 * 4 + sizeof(cornetto_ivl_t)) + 16);
        u64 *d_small = (u64 *)cn_ws(h, WS_TB_SMALL, 64);
        u64 *p_small = (u64 *)cn_pin(h, PIN_SMALL, 64);
        if (!d_flag || !d_small || !p_small) return cn_fail(h, CORNETTO_E_NOMEM, "%s: workspace allocation failed", who);
        uint32_t *d_rank = d_flag + n_sd;
        cornetto_ivl_t *d_out = reinterpret_cast<cornetto_ivl_t *>(d_rank + n_sd);
        BkArgs A{d_len, n_ctg, d_sd, n_sd, d_flag, d_rank, d_small, reinterpret_cast<uint32_t *>(d_small + 1), d_out};
        const unsigned nb = (unsigned)((n_sd + 255) / 256);
        CN_HIP(h, hipMemsetAsync(d_small, 0, 64, h->stream));
        CN_LAUNCH(h, "bk_check", bk_check<<<dim3(nb), dim3(256), 0, h->stream>>>(A));
        if (n_rows > 0)
            CN_LAUNCH(h, "bk_mark", bk_mark<<<dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, h->stream>>>(A, reinterpret_cast<const int4 *>(d_rows), n_rows, hits));
        CN_TRY(cnscan::exclusive_u32(h, "bk_scan", d_flag, n_sd, 1, d_rank, d_small));
        CN_LAUNCH(h, "bk_emit", bk_emit<<<dim3(nb), dim3(256), 0, h->stream>>>(A));
        CN_HIP(h, hipMemcpyAsync(p_small, d_small, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        const uint32_t err = (uint32_t)(p_small[0] >> 32);
        if (err & BK_E_ORDER)
            return cn_fail(h, bad_list, "%s: the low-complexity intervals are not in (contig, start) order with a gap between two of them, or name a contig outside the table", who);
        if (err)
            return cn_fail(h, CORNETTO_E_FORMAT, "%s: %s with coordinates outside its contig (the reference indexes its bitset unchecked)", who,
                           (err & BK_E_IVL) ? "low-complexity interval" : "telomere row");
        n = (int64_t)(p_small[0] & 0xFFFFFFFFull);
        if (n > n_sd) return cn_fail(h, CORNETTO_E_HIP, "%s: %lld marked intervals of %lld", who, (long long)n, (long long)n_sd);
        if (n > 0) {
            o = (cornetto_ivl_t *)cn_result_alloc((size_t)n * sizeof(cornetto_ivl_t));
            if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "%s: host allocation failed", who);
            if (hipMemcpyAsync(o, d_out, (size_t)n * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
                cornetto_free(o);
                return cn_fail(h, CORNETTO_E_HIP, "%s: copying the records back failed", who);
            }
        }
    }
    if (!o) {
        o = (cornetto_ivl_t *)malloc(sizeof(cornetto_ivl_t));
        if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "%s: host allocation failed", who);
    }
    *out = o;
    *n_out = n;
    return CORNETTO_OK;
}

}  // namespace

extern "C" {

int cornetto_telo_breaks(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, int32_t T, int32_t W, cornetto_ivl_t **rows, int64_t *n_rows)
{
    if (!h || !a || !motif || !rows || !n_rows) return cn_fail(h, CORNETTO_E_ARG, "telo_breaks: bad argument");
    *rows = nullptr;
    *n_rows = 0;
    CN_HIP(h, hipSetDevice(h->device));
    cn_sdust_drop_pending(h);                          // (it ends with a timing bracket of its own: in front of this call's)
    cn_timing_begin(h);
    const cornetto_ivl_t *d_sd = nullptr;
    const cornetto_hit_t *d_hits = nullptr;
    int64_t n_sd = 0, n_hits = 0;
    int rc = cn_sdust_list_impl(h, a, T, W, &d_sd, &n_sd);
    if (rc == CORNETTO_OK) rc = cn_telo_hits_impl(h, a, motif, &d_hits, &n_hits);        // (its workspaces are not sdust's: d_sd stays)
    if (rc == CORNETTO_OK) rc = bk_stage(h, "telo_breaks", a->d_len, a->n, d_sd, n_sd, d_hits, n_hits, 1, CORNETTO_E_HIP, rows, n_rows);
    cn_timing_end(h);
    return rc;
}

int cornetto_telobreaks_ivl(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *sd, int64_t n_sd, const cornetto_telrow_t *tel, int64_t n_tel,
                            cornetto_ivl_t **out, int64_t *n_out)
{
    if (!h || !out || !n_out || n_ctg < 0 || n_sd < 0 || n_tel < 0 || (n_ctg > 0 && !ctg_len) || (n_sd > 0 && !sd) || (n_tel > 0 && !tel))
        return cn_fail(h, CORNETTO_E_ARG, "telobreaks_ivl: bad argument");
    *out = nullptr;
    *n_out = 0;
    for (int32_t c = 0; c < n_ctg; ++c)
        if (ctg_len[c] < 0) return cn_fail(h, CORNETTO_E_ARG, "telobreaks_ivl: contig %d has a negative length", c);
    CN_HIP(h, hipSetDevice(h->device));
    // lengths | intervals | rows, as the caller gave them
    const size_t b_len = ((size_t)n_ctg * 4 + 15) & ~(size_t)15, b_sd = ((size_t)n_sd * sizeof(cornetto_ivl_t) + 15) & ~(size_t)15;
    uint8_t *ws = (uint8_t *)cn_ws(h, WS_TB, b_len + b_sd + (size_t)n_tel * sizeof(cornetto_telrow_t) + 16);
    if (!ws) return cn_fail(h, CORNETTO_E_NOMEM, "telobreaks_ivl: workspace allocation failed");
    cn_timing_begin(h);
    int32_t *d_len = reinterpret_cast<int32_t *>(ws);
    cornetto_ivl_t *d_sd = reinterpret_cast<cornetto_ivl_t *>(ws + b_len);
    cornetto_telrow_t *d_tel = reinterpret_cast<cornetto_telrow_t *>(ws + b_len + b_sd);
    // (the arrays are the caller's: whatever happens, nothing returns before the stream has drained)
    int rc = [&]() -> int {
        if (n_ctg > 0) CN_HIP(h, hipMemcpyAsync(d_len, ctg_len, (size_t)n_ctg * 4, hipMemcpyHostToDevice, h->stream));
        if (n_sd > 0) CN_HIP(h, hipMemcpyAsync(d_sd, sd, (size_t)n_sd * sizeof(cornetto_ivl_t), hipMemcpyHostToDevice, h->stream));
        if (n_tel > 0) CN_HIP(h, hipMemcpyAsync(d_tel, tel, (size_t)n_tel * sizeof(cornetto_telrow_t), hipMemcpyHostToDevice, h->stream));
        return bk_stage(h, "telobreaks_ivl", d_len, n_ctg, d_sd, n_sd, d_tel, n_tel, 0, CORNETTO_E_ARG, out, n_out);
    }();
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == CORNETTO_OK) {            // (an empty interval list: bk_stage queued nothing behind the uploads)
        cornetto_free(*out);
        *out = nullptr;
        *n_out = 0;
        rc = cn_fail(h, CORNETTO_E_HIP, "telobreaks_ivl: the uploads failed");
    }
    cn_timing_end(h);
    return rc;
}

}  // extern "C"
