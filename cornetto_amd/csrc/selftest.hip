// selftest.hip — the scan primitives of wave.hpp / scan.hpp / ivlmerge.hpp and the radix sort of sort.hpp behind plain C entry points, DEVELOPMENT BUILD ONLY (-DCN_DEV:
// the product object of this file is empty, tests/test_abi.py looks for the prefix in both libraries).  tests/test_gpu_scan.py
// (tests/selftest_bind.py) compares them with numpy on inputs the product entry points cannot produce: prepared tile states for the
// look-back, full-range values, strides and counter sets at more than one tile, epochs next to the wrap.  cn_selftest_ws_fill sets the
// contents of the handle's workspaces between two calls (tests/test_gpu_ws_fill.py: no stage depends on what they held); cn_selftest_telo_marks brings the
// mark bitmap of the telofind pass to the host (tests/test_gpu_telofind_seams.py compares it word by word).  Not part of the C ABI: no
// declaration in include/cornetto_accel.h.  Every entry takes host pointers, allocates, copies and synchronises by itself.
#ifdef CN_DEV
#include "common.hpp"
#include "internal.hpp"
#include "ivlmerge.hpp"
#include "scan.hpp"
#include "sort.hpp"
#include "wave.hpp"

namespace {

using u64 = unsigned long long;

// one value per lane, one wave per 64 values
template <int WHICH>
__global__ __launch_bounds__(256) void selftest_wave(const void *in, void *out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;                                // (n is a multiple of 64: whole waves leave)
    const int lane = threadIdx.x & 63;
    if (WHICH == 0) static_cast<uint32_t *>(out)[i] = cnwave::wave_incl<uint32_t>(static_cast<const uint32_t *>(in)[i], lane);
    if (WHICH == 1) static_cast<u64 *>(out)[i] = cnwave::wave_incl<u64>(static_cast<const u64 *>(in)[i], lane);
    if (WHICH == 2) static_cast<uint32_t *>(out)[i] = cnwave::wave_incl_dpp(static_cast<const uint32_t *>(in)[i]);
    if (WHICH == 3) static_cast<uint32_t *>(out)[i] = cnwave::wave_sum(static_cast<const uint32_t *>(in)[i]);
}

// one value per thread, one block_excl per workgroup (and per kernel)
template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void selftest_block_excl(const T *in, T *pre, T *totals)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    T total;
    pre[i] = cnscan::block_excl<T, THREADS>(in[i], total);
    if (threadIdx.x == THREADS - 1) totals[blockIdx.x] = total;
}

// ONE wave walks over prepared states
__global__ __launch_bounds__(64) void selftest_walk(u64 *st, int64_t stride, int64_t tile, uint32_t epoch, uint32_t own, uint32_t *out)
{
    const uint32_t excl = cnscan::lookback_excl(st, stride, tile, epoch, own, (int)threadIdx.x);
    if (threadIdx.x == 0) *out = excl;
}

// The look-back of scan.hpp restated on the host: true when the walk of `tile` over these words ENDS — every word that a round it
// reaches polls carries the epoch and a kind, so no poll is repeated.  (A word that is not ready makes the wave spin until somebody
// writes it, and nobody would.)
bool walk_ends(const u64 *w, int64_t stride, int64_t tile, uint32_t epoch)
{
    const u64 tag = (u64)(epoch & 0x3FFFFFFFu) << 32;
    for (int64_t pos = tile - 1; tile > 0; pos -= 64) {
        bool incl = false;
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t idx = pos - lane;
            if (idx < 0) {                             // the sentinel: an inclusive prefix of 0
                incl = true;
                continue;
            }
            const u64 x = w[idx * stride];
            if ((x >> 62) == 0 || (x & (0x3FFFFFFFull << 32)) != tag) return false;
            if ((x >> 62) == 2) incl = true;
        }
        if (incl) break;
    }
    return true;
}

template <typename T, int THREADS>
int run_block_excl(cornetto_accel_t *h, const void *in, void *pre_out, void *totals_out, int64_t n_blocks)
{
    const size_t n = (size_t)n_blocks * THREADS;
    DevBuf d_in, d_pre, d_tot;
    if (d_in.alloc(n * sizeof(T)) != hipSuccess || d_pre.alloc(n * sizeof(T)) != hipSuccess || d_tot.alloc((size_t)n_blocks * sizeof(T)) != hipSuccess)
        return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_in.p, in, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    selftest_block_excl<T, THREADS><<<dim3((unsigned)n_blocks), dim3(THREADS), 0, h->stream>>>(d_in.as<T>(), d_pre.as<T>(), d_tot.as<T>());
    CN_HIP(h, hipGetLastError());
    CN_HIP(h, hipMemcpyAsync(pre_out, d_pre.p, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipMemcpyAsync(totals_out, d_tot.p, (size_t)n_blocks * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    return CORNETTO_OK;
}

// ---- what a workspace slot holds between two complete calls (DESIGN.md section 3 has the same table, with the owning stages) -----------------
//   scratch   nothing: every word a call reads it has written itself (cn_ws: "contents undefined")
//   vouched   contents a later call may use again, but only while the named host fields of the handle say so
//   polled    words that kernels wait on (the epoch-tagged tile states of the single-pass scans); valid by epoch, never by content
enum WsClass { WSC_SCRATCH, WSC_VOUCHED, WSC_POLLED };
struct WsRow {
    int slot;
    const char *name;
    WsClass cls;
    const char *voucher;           // vouched: the host fields; polled: what makes a word count
};
#define WS_ROW(s, c, v) {s, #s, c, v}
#define WS_SCR(s) {s, #s, WSC_SCRATCH, ""}
constexpr WsRow ws_table[] = {
    WS_ROW(WS_TF_LUT, WSC_VOUCHED, "tf_lut_key, tf_lut_ptr"),
    WS_SCR(WS_TF_CNT), WS_SCR(WS_TF_TB), WS_SCR(WS_TF_TC), WS_SCR(WS_TF_L0), WS_SCR(WS_TF_L1), WS_SCR(WS_TF_L2), WS_SCR(WS_TF_L3),
    WS_ROW(WS_TF_BITMAP, WSC_VOUCHED, "tf_bm_uid, tf_bm_ptr, tf_bm_words"),
    WS_SCR(WS_TF_ROFF), WS_SCR(WS_TF_RUNS), WS_SCR(WS_TF_NRUNS),
    WS_SCR(WS_TW_BOFF), WS_SCR(WS_TW_TILES), WS_SCR(WS_TW_OUT), WS_SCR(WS_TW_CNT), WS_SCR(WS_TW_HITS), WS_SCR(WS_TW_LEN), WS_SCR(WS_TW_BITMAP),
    WS_SCR(WS_SD_OUT), WS_SCR(WS_SD_CNT), WS_SCR(WS_SD_OFF), WS_SCR(WS_SD_DST), WS_SCR(WS_SD_STATS), WS_SCR(WS_SD_PERM),
    WS_SCR(WS_CB_T32), WS_SCR(WS_CB_T64), WS_SCR(WS_CB_GRAND),
    WS_SCR(WS_CW_REGS), WS_SCR(WS_CW_SEL), WS_SCR(WS_CW_CNT), WS_SCR(WS_CW_TRES), WS_SCR(WS_CW_CF),
    WS_SCR(WS_TF_HITS),
    WS_SCR(WS_BG_TEXT_A), WS_SCR(WS_BG_TEXT_B), WS_SCR(WS_BG_TOK_A), WS_SCR(WS_BG_TOK_B), WS_SCR(WS_BG_CNT_A), WS_SCR(WS_BG_CNT_B), WS_SCR(WS_BG_SMALL), WS_SCR(WS_BG_BRK),
    WS_SCR(WS_TB), WS_SCR(WS_TB_SMALL), WS_SCR(WS_TB_OUT), WS_SCR(WS_CW_MERGE), WS_SCR(WS_IVL_MERGE),
    WS_SCR(WS_FQ_TEXT), WS_SCR(WS_FQ_CNT), WS_SCR(WS_FQ_NL), WS_SCR(WS_FQ_RECS), WS_SCR(WS_FQ_ENDS), WS_SCR(WS_FQ_SRC),
    WS_ROW(WS_SCAN, WSC_POLLED, "scan_epoch, scan_tickets"),
    WS_ROW(WS_STITCH, WSC_POLLED, "st_epoch, st_tickets"),
    WS_SCR(WS_TE_WORDS), WS_SCR(WS_TE_REG), WS_SCR(WS_TE_ROWS), WS_SCR(WS_TE_CNT),
    WS_SCR(WS_SORT), WS_SCR(WS_HAP_ROWS), WS_SCR(WS_HAP_BLOCKS), WS_SCR(WS_HAP_FUN),
    WS_SCR(WS_BZ_BLOCKS), WS_SCR(WS_BZ_STATUS), WS_SCR(WS_BZ_PACK),
    WS_SCR(WS_DF_STAGE), WS_SCR(WS_DF_SIZE), WS_SCR(WS_DF_TOTAL),
    WS_SCR(WS_KQ_CNT), WS_SCR(WS_KQ_MAP), WS_SCR(WS_KQ_ROWS),
    WS_SCR(WS_KT_CNT), WS_SCR(WS_KT_MAP),
    WS_SCR(WS_KC_HIST),
};
#undef WS_ROW
#undef WS_SCR
static_assert(sizeof(ws_table) / sizeof(ws_table[0]) == WS_COUNT, "every device workspace slot has a class: a new slot gets a row here and in DESIGN.md section 3");
constexpr bool ws_table_in_order()
{
    for (int i = 0; i < WS_COUNT; ++i)
        if (ws_table[i].slot != i) return false;
    return true;
}
static_assert(ws_table_in_order(), "the rows of ws_table stand in the order of the enum");

// the pinned slots: all scratch (the host reads of a call what the call's own copies wrote)
constexpr const char *pin_names[] = {"PIN_A", "PIN_B", "PIN_C", "PIN_D", "PIN_E", "PIN_F", "PIN_SMALL", "PIN_TW", "PIN_CW", "PIN_STEP", "PIN_TE"};
static_assert(sizeof(pin_names) / sizeof(pin_names[0]) == PIN_COUNT, "every pinned slot has a name");

}  // namespace

extern "C" {

// the name of device slot `slot` / of pinned slot `slot` as the enums of common.hpp spell it; null outside the enum
const char *cn_selftest_ws_name(int slot) { return slot >= 0 && slot < WS_COUNT ? ws_table[slot].name : nullptr; }
const char *cn_selftest_pin_name(int slot) { return slot >= 0 && slot < PIN_COUNT ? pin_names[slot] : nullptr; }
// 0 scratch, 1 vouched, 2 polled (-1 outside the enum); *voucher: the host fields that vouch ("" for scratch)
int cn_selftest_ws_class(int slot, const char **voucher)
{
    if (slot < 0 || slot >= WS_COUNT) return -1;
    if (voucher) *voucher = ws_table[slot].voucher;
    return (int)ws_table[slot].cls;
}

// Every byte of every allocated workspace of the handle set to `byte`, over the slot's whole capacity: what the next call finds where cn_ws says
// "contents undefined".  Scratch slots and the pinned slots are filled; vouched slots are filled and their voucher is dropped exactly as a fresh
// handle has it (the next call uploads / clears again); polled slots (WS_SCAN, WS_STITCH) are NOT touched — their words are waited on by kernels, a
// filled word with the epoch of a later call would be waited on for ever; tests/test_gpu_scan.py owns them.  No word any kernel spins on is written.
// filled[s] / skipped[s] (n_dev >= WS_COUNT entries each), pin_filled[s] (n_pin >= PIN_COUNT): bytes per slot.
// BETWEEN COMPLETE OPERATIONS ONLY: CORNETTO_E_ARG, and nothing touched, while cornetto_sdust_asm_begin() waits for its _end or a lazy handle's copies
// are out.  What the handle cannot tell is the caller's to keep: no fill while a streaming session (cornetto_bgin_*, cornetto_bgrun_*) has a feed or a
// prefetch on its way or a text object's slabs are in flight on its own queues (only the handle's three streams are waited for here); the tests fill
// between complete sessions.
int cn_selftest_ws_fill(cornetto_accel_t *h, int byte, int64_t *filled, int64_t *skipped, int n_dev, int64_t *pin_filled, int n_pin)
{
    if (!h || byte < 0 || byte > 255 || !filled || !skipped || n_dev < WS_COUNT || !pin_filled || n_pin < PIN_COUNT) return cn_fail(h, CORNETTO_E_ARG, "selftest_ws_fill: bad argument");
    if (h->sd_pend.state != 0 || h->copies_pending) return cn_fail(h, CORNETTO_E_ARG, "selftest_ws_fill: an operation is in flight on the handle");
    CN_HIP(h, hipSetDevice(h->device));
    auto sync_all = [&]() -> int {
        CN_HIP(h, hipStreamSynchronize(h->stream));
        if (h->stream2) CN_HIP(h, hipStreamSynchronize(h->stream2));
        if (h->copy_stream) CN_HIP(h, hipStreamSynchronize(h->copy_stream));
        return CORNETTO_OK;
    };
    CN_TRY(sync_all());
    for (int s = 0; s < WS_COUNT; ++s) {
        const cornetto_accel::Ws &w = h->dev[s];
        filled[s] = skipped[s] = 0;
        if (!w.p || !w.bytes) continue;
        if (ws_table[s].cls == WSC_POLLED) {
            skipped[s] = (int64_t)w.bytes;
            continue;
        }
        CN_HIP(h, hipMemsetAsync(w.p, byte, w.bytes, h->stream));
        filled[s] = (int64_t)w.bytes;
        if (s == WS_TF_LUT) {                         // (telo.hip: the tables of a motif are uploaded unless these say they are there)
            h->tf_lut_key.clear();
            h->tf_lut_ptr = nullptr;
        }
        if (s == WS_TF_BITMAP) {                      // (telo.hip: the padding words are cleared unless these say they are zero)
            h->tf_bm_uid = 0;
            h->tf_bm_ptr = nullptr;
            h->tf_bm_words = 0;
        }
    }
    for (int s = 0; s < PIN_COUNT; ++s) {
        const cornetto_accel::Ws &w = h->pin[s];
        pin_filled[s] = 0;
        if (!w.p || !w.bytes) continue;
        memset(w.p, byte, w.bytes);
        pin_filled[s] = (int64_t)w.bytes;
    }
    return sync_all();
}

// out[i] = the primitive `which` over the wave of in[i]: 0 wave_incl<uint32_t>, 1 wave_incl<unsigned long long> (in and out 64-bit),
// 2 wave_incl_dpp, 3 wave_sum.  n: a multiple of 64.
int cn_selftest_wave(cornetto_accel_t *h, int which, const void *in, void *out, int64_t n)
{
    if (!h || !in || !out || n <= 0 || n % 64 || which < 0 || which > 3) return cn_fail(h, CORNETTO_E_ARG, "selftest_wave: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)n * (which == 1 ? 8 : 4);
    DevBuf d_in, d_out;
    if (d_in.alloc(bytes) != hipSuccess || d_out.alloc(bytes) != hipSuccess) return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_in.p, in, bytes, hipMemcpyHostToDevice, h->stream));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (which == 0) selftest_wave<0><<<grid, block, 0, h->stream>>>(d_in.p, d_out.p, n);
    if (which == 1) selftest_wave<1><<<grid, block, 0, h->stream>>>(d_in.p, d_out.p, n);
    if (which == 2) selftest_wave<2><<<grid, block, 0, h->stream>>>(d_in.p, d_out.p, n);
    if (which == 3) selftest_wave<3><<<grid, block, 0, h->stream>>>(d_in.p, d_out.p, n);
    CN_HIP(h, hipGetLastError());
    CN_HIP(h, hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    return CORNETTO_OK;
}

// pre_out[b * threads + t], totals_out[b] = block_excl<T, threads> of in[b * threads + t]; threads: 256 or 1024; T: 64-bit when is64
int cn_selftest_block_excl(cornetto_accel_t *h, int threads, int is64, const void *in, void *pre_out, void *totals_out, int64_t n_blocks)
{
    if (!h || !in || !pre_out || !totals_out || n_blocks <= 0 || n_blocks > 65536 || (threads != 256 && threads != 1024))
        return cn_fail(h, CORNETTO_E_ARG, "selftest_block_excl: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    if (threads == 256) return is64 ? run_block_excl<u64, 256>(h, in, pre_out, totals_out, n_blocks) : run_block_excl<uint32_t, 256>(h, in, pre_out, totals_out, n_blocks);
    return is64 ? run_block_excl<u64, 1024>(h, in, pre_out, totals_out, n_blocks) : run_block_excl<uint32_t, 1024>(h, in, pre_out, totals_out, n_blocks);
}

// cnscan::lookback_excl by one wave over the prepared states `words` (updated in place), the state of tile t at words[t * stride + stride - 1]
// (stride 1: scan_lookback's layout; stride 4: st_fused's, the head count's state is the fourth word of a tile's record).
// CORNETTO_E_ARG, and NO launch, unless the walk provably ends on these words (walk_ends above).
int cn_selftest_walk(cornetto_accel_t *h, unsigned long long *words, int64_t n_words, int64_t stride, int64_t tile, uint32_t epoch, uint32_t own, uint32_t *excl_out)
{
    if (!h || !words || !excl_out || stride < 1 || stride > 64 || tile < 0 || tile > (1 << 20) || n_words < (tile + 1) * stride)
        return cn_fail(h, CORNETTO_E_ARG, "selftest_walk: bad argument");
    if (!walk_ends(words + (stride - 1), stride, tile, epoch))
        return cn_fail(h, CORNETTO_E_ARG, "selftest_walk: a state the walk of tile %lld polls is not ready: it would not end", (long long)tile);
    CN_HIP(h, hipSetDevice(h->device));
    DevBuf d_w, d_o;
    if (d_w.alloc((size_t)n_words * 8) != hipSuccess || d_o.alloc(8) != hipSuccess) return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_w.p, words, (size_t)n_words * 8, hipMemcpyHostToDevice, h->stream));
    selftest_walk<<<dim3(1), dim3(64), 0, h->stream>>>(d_w.as<u64>() + (stride - 1), stride, tile, epoch, own, d_o.as<uint32_t>());
    CN_HIP(h, hipGetLastError());
    CN_HIP(h, hipMemcpyAsync(words, d_w.p, (size_t)n_words * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipMemcpyAsync(excl_out, d_o.p, 4, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    return CORNETTO_OK;
}

// cnscan::exclusive_u32_multi itself, on the handle's own WS_SCAN, epoch and tickets: in holds n records of `stride` words, counter q is
// word first + q of a record (first + m <= stride); outs: m arrays of n words one after the other; totals: m x u64, or null
int cn_selftest_scan_u32(cornetto_accel_t *h, const uint32_t *in, int64_t n, int stride, int first, int m, uint32_t *outs, unsigned long long *totals)
{
    if (!h || !in || !outs || n <= 0 || n > ((int64_t)1 << 28) || stride < 1 || first < 0 || m < 1 || m > 4 || first + m > stride)
        return cn_fail(h, CORNETTO_E_ARG, "selftest_scan_u32: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    DevBuf d_in, d_out, d_tot;
    if (d_in.alloc((size_t)n * stride * 4) != hipSuccess || d_out.alloc((size_t)n * m * 4) != hipSuccess || d_tot.alloc(4 * 8) != hipSuccess)
        return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_in.p, in, (size_t)n * stride * 4, hipMemcpyHostToDevice, h->stream));
    uint32_t *o[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int q = 0; q < m; ++q) o[q] = d_out.as<uint32_t>() + (size_t)q * n;
    CN_TRY(cnscan::exclusive_u32_multi(h, "selftest_scan", d_in.as<uint32_t>() + first, n, stride, m, o, totals ? d_tot.as<u64>() : nullptr));
    CN_HIP(h, hipMemcpyAsync(outs, d_out.p, (size_t)n * m * 4, hipMemcpyDeviceToHost, h->stream));
    if (totals)
        CN_HIP(h, hipMemcpyAsync(totals, d_tot.p, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    return CORNETTO_OK;
}

// the host's epoch of the scans / of the fused merge alone: the ticket bases stay in step with the device's counters
int cn_selftest_scan_set_epoch(cornetto_accel_t *h, uint32_t epoch)
{
    if (!h) return CORNETTO_E_ARG;
    h->scan_epoch = epoch;
    return CORNETTO_OK;
}

int cn_selftest_st_set_epoch(cornetto_accel_t *h, uint32_t epoch)
{
    if (!h) return CORNETTO_E_ARG;
    h->st_epoch = epoch;
    return CORNETTO_OK;
}

// cnivl::merge_fused itself (no public entry point reaches it without sdust in front), on the handle's own WS_STITCH, epoch and tickets:
// in[0 .. n) ordered by (contig, start) -> out[0 .. *n_out), out with room for n rows; the grid is sized for n_cap >= n rows
int cn_selftest_merge_fused(cornetto_accel_t *h, const cornetto_ivl_t *in, int64_t n, int64_t n_cap, int32_t dist, cornetto_ivl_t *out, int64_t *n_out)
{
    if (!h || !in || !out || !n_out || n <= 0 || n_cap < n || n_cap > ((int64_t)1 << 28) || dist < 0) return cn_fail(h, CORNETTO_E_ARG, "selftest_merge_fused: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    DevBuf d_in, d_out, d_small;
    if (d_in.alloc((size_t)n_cap * sizeof(cornetto_ivl_t)) != hipSuccess || d_out.alloc((size_t)n_cap * sizeof(cornetto_ivl_t)) != hipSuccess || d_small.alloc(16) != hipSuccess)
        return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    unsigned long long small[2] = {(unsigned long long)n, ~0ull};       // the number of rows | the count (kept when the merge declines)
    CN_HIP(h, hipMemcpyAsync(d_in.p, in, (size_t)n * sizeof(cornetto_ivl_t), hipMemcpyHostToDevice, h->stream));
    CN_HIP(h, hipMemcpyAsync(d_small.p, small, 16, hipMemcpyHostToDevice, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));                         // (`small` is pageable memory of this frame)
    CN_TRY(cnivl::merge_fused(h, "selftest_merge", d_in.as<cornetto_ivl_t>(), d_small.as<u64>(), n_cap, dist, d_out.as<cornetto_ivl_t>(), d_small.as<u64>() + 1));
    CN_HIP(h, hipMemcpyAsync(small, d_small.p, 16, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    if (small[1] > (unsigned long long)n) return cn_fail(h, CORNETTO_E_HIP, "selftest_merge_fused: no count");
    CN_HIP(h, hipMemcpyAsync(out, d_out.p, (size_t)small[1] * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    *n_out = (int64_t)small[1];
    return CORNETTO_OK;
}

// cnsort::pairs_u64 itself, on the handle's own WS_SORT (and WS_SCAN, through the table's scan): the n pairs (keys[i], vals[i]) -> the same
// pairs in ascending key order, equal keys in input order; key_bits: the digits that are looked at (the keys are 0 above)
int cn_selftest_sort_pairs(cornetto_accel_t *h, const unsigned long long *keys, const uint32_t *vals, int64_t n, int key_bits, unsigned long long *out_keys,
                           uint32_t *out_vals)
{
    if (!h || n < 0 || n > ((int64_t)1 << 28) || (n > 0 && (!keys || !vals || !out_keys || !out_vals)) || key_bits < 1 || key_bits > 64)
        return cn_fail(h, CORNETTO_E_ARG, "selftest_sort_pairs: bad argument");
    if (n == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    DevBuf d_k, d_v;
    if (d_k.alloc((size_t)n * 8) != hipSuccess || d_v.alloc((size_t)n * 4) != hipSuccess) return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    uint8_t *ws = (uint8_t *)cn_ws(h, WS_SORT, cnsort::ws_bytes(n));
    if (!ws) return cn_fail(h, CORNETTO_E_NOMEM, "selftest: workspace allocation failed");
    CN_HIP(h, hipMemcpyAsync(d_k.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    CN_HIP(h, hipMemcpyAsync(d_v.p, vals, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    u64 *r_k = nullptr;
    uint32_t *r_v = nullptr;
    CN_TRY(cnsort::pairs_u64(h, "selftest_sort", d_k.as<u64>(), d_v.as<uint32_t>(), n, ws, key_bits, &r_k, &r_v));
    CN_HIP(h, hipMemcpyAsync(out_keys, r_k, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipMemcpyAsync(out_vals, r_v, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    return CORNETTO_OK;
}

// cn_telo_marks_impl itself (internal.hpp: what cornetto_telo_ends builds its regions from), the words brought to the host: a motif without a
// border takes tf_scan's own marks in its count-only mode, one with a border or beyond the automaton the marked runs.  words_out[0 .. n_words):
// the contigs back to back, every contig from a multiple of 64 bits, n_words = the sum of ceil(len / 64) — anything else is CORNETTO_E_ARG
int cn_selftest_telo_marks(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, unsigned long long *words_out, int64_t n_words)
{
    if (!h || !a || !motif || n_words < 0 || (n_words > 0 && !words_out)) return cn_fail(h, CORNETTO_E_ARG, "selftest_telo_marks: bad argument");
    int64_t want = 0;
    for (int32_t c = 0; c < a->n; ++c) want += ((int64_t)a->len[c] + 63) / 64;
    if (n_words != want) return cn_fail(h, CORNETTO_E_ARG, "selftest_telo_marks: %lld words asked for, the assembly has %lld", (long long)n_words, (long long)want);
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const unsigned long long *d_marks = nullptr;
    const int rc = [&]() -> int {
        CN_TRY(cn_telo_marks_impl(h, a, motif, &d_marks));
        if (n_words > 0) {
            if (!d_marks) return cn_fail(h, CORNETTO_E_HIP, "selftest_telo_marks: no marks");
            CN_HIP(h, hipMemcpyAsync(words_out, d_marks, (size_t)n_words * 8, hipMemcpyDeviceToHost, h->stream));
        }
        CN_HIP(h, hipStreamSynchronize(h->stream));
        return CORNETTO_OK;
    }();
    cn_timing_end(h);                                  // (on an error as well: the events go back to the pool)
    return rc;
}

}  // extern "C"
#endif
