// fqseq.hip — the length-filtered text `seq` prints, from FASTQ text on the device (include/cornetto_accel.h: cornetto_fqseq_*).  The text of a
// feed — plain bytes from the host, or the next BGZF blocks of the file, inflated here (cn_bgzf_inflate_raw) — lands behind the tail the last
// window left; per window:
//   fq_nl_count / fq_scan / fq_nl_scatter   (marks.hpp) the newline index
//   fq_records    (fqrec.hpp: the rules of cornetto_fastq_split, not a copy of them) a thread per four lines: the record, the first group that
//                 is not a plain record
//   fqseq_zero    the first byte 0 of the window (16 bytes per thread); fqseq_fold: its record joins "the first group that is not plain" — the
//                 reference prints with printf("%s"), so a record with a byte 0 is the sequential reader's
//   with cornetto_fqseq_set_max_err() (`seq -q`; nothing of it runs or is allocated otherwise)
//     fqseq_qrange  a thread per record: its quality line as a range of qmean_sum, of length 0 where -m has dropped it
//     qmean_sum     (qmean.hip) the sums of quality weights, into a table the window zeroes itself
//     fqseq_qkeep   a thread per record: sum > P * len clears `keep`; the reads and bases that stay are counted, the ones that go are added
//                   to the counts of `reads >= min_len` here, since fqseq_size below counts what is still kept
//   fqseq_size    a thread per record: the bytes of its text (0: dropped by -m), the counts of the two summary lines (a 64-bit atomic per wave)
//   fqseq_scan    the exclusive scan of the sizes (the look-back of scan.hpp): every record's offset in the window's text
// and per get of bytes [at, at + n) of that text
//   fqseq_text    emit.hip's decomposition: a workgroup writes a tile of consecutive output bytes, a thread 16 bytes with one aligned vector
//                 store.  The tile's records come from a binary search of the offset table, once per tile; a chunk that lies inside the name,
//                 the comment, the bases or the qualities of one record is a misaligned 16-byte copy (two aligned loads and a byte funnel),
//                 every other chunk (the '@', the tab, the newlines, "+", a record border, the end of the range) goes byte by byte.
// or, for cornetto_fqseq_get_bgzf(), behind fqseq_text on the slab
//   bgzf_deflate / bgzf_scan / bgzf_pack   (deflate.hip) the slab's text as BGZF members, packed: only those cross the bus.
// Sizes are 32-bit: a window has at most 2^32-256 bytes and a record prints at most one byte more than it has (a last line without its
// newline), so the text of a window is below 2^32.
#include "bgtok.hpp"
#include "common.hpp"
#include "deflate.hpp"
#include "fqrec.hpp"
#include "fqseq.hpp"
#include "internal.hpp"
#include "marks.hpp"
#include "scan.hpp"

namespace {

constexpr int FX_THREADS = 256;
constexpr int FX_PER_THREAD = 4;                                          // 16-byte chunks per thread
constexpr int64_t FX_TILE = (int64_t)FX_THREADS * 16 * FX_PER_THREAD;     // 16 KiB of output per block
static_assert(FX_TILE == CORNETTO_FQSEQ_TILE, "the tile the tests plant their seams at");

// words of the small device block
enum { SM_BAD = 0 /* u32 first group not plain, u32 first byte 0 */, SM_TOTAL_N = 1, SM_TOTAL_B = 2, SM_KEPT_N = 3, SM_KEPT_B = 4, SM_TEXT = 5, SM_Q_N = 6, SM_Q_B = 7, SM_WORDS = 8 };

__global__ void __launch_bounds__(cnmarks::MK_THREADS) fqseq_zero(const uint8_t *__restrict__ text, int64_t n, uint32_t *first_zero)
{
    const int64_t pos = ((int64_t)blockIdx.x * cnmarks::MK_THREADS + threadIdx.x) * 16;
    if (pos >= n) return;
    const uint32_t m = byte_mask16<0>(text, pos, n);
    if (m) atomicMin(first_zero, (uint32_t)(pos + (__ffs((int)m) - 1)));
}

// the record that holds the first byte 0 is not plain for this stage (a byte 0 behind the last whole record belongs to no record yet)
__global__ void __launch_bounds__(64) fqseq_fold(const uint32_t *__restrict__ first_zero, const uint32_t *__restrict__ ends, int64_t n_rec, uint32_t *first_bad)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t z = *first_zero;
    if (z == 0xFFFFFFFFu) return;
    int64_t lo = 0, hi = n_rec;          // the first record whose end lies behind z
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ends[mid] > z) hi = mid;
        else lo = mid + 1;
    }
    if (lo < n_rec) atomicMin(first_bad, (uint32_t)lo);
}

__device__ __forceinline__ unsigned long long fx_wave_sum(unsigned long long s)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__global__ void __launch_bounds__(256) fqseq_size(const cornetto_fqrec_t *__restrict__ recs, int64_t n_rec, uint32_t *__restrict__ size, unsigned long long *sm)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long tn = 0, tb = 0, kn = 0, kb = 0;
    if (r < n_rec) {
        const cornetto_fqrec_t x = recs[r];
        tn = 1;
        tb = (unsigned long long)x.len;
        if (x.keep) {
            kn = 1;
            kb = tb;
        }
        size[r] = fx_size(x);
    }
    tn = fx_wave_sum(tn);
    tb = fx_wave_sum(tb);
    kn = fx_wave_sum(kn);
    kb = fx_wave_sum(kb);
    if ((threadIdx.x & 63) == 0 && tn) {
        atomicAdd(sm + SM_TOTAL_N, tn);
        atomicAdd(sm + SM_TOTAL_B, tb);
        if (kn) {
            atomicAdd(sm + SM_KEPT_N, kn);
            atomicAdd(sm + SM_KEPT_B, kb);
        }
    }
}

__global__ void __launch_bounds__(256) fqseq_qrange(const cornetto_fqrec_t *__restrict__ recs, int64_t n_rec, uint32_t *__restrict__ start, uint32_t *__restrict__ len)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const cornetto_fqrec_t x = recs[r];
    start[r] = (uint32_t)x.qual;
    len[r] = x.keep ? (uint32_t)x.len : 0u;
}

__global__ void __launch_bounds__(256) fqseq_qkeep(cornetto_fqrec_t *__restrict__ recs, int64_t n_rec, const unsigned long long *__restrict__ sum, int64_t max_err,
                                                   unsigned long long *sm)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long dn = 0, db = 0, pn = 0, pb = 0;
    if (r < n_rec && recs[r].keep) {
        const unsigned long long len = (unsigned long long)recs[r].len;
        if (sum[r] > (unsigned long long)max_err * len) {
            recs[r].keep = 0;
            dn = 1;
            db = len;
        } else {
            pn = 1;
            pb = len;
        }
    }
    dn = fx_wave_sum(dn);
    db = fx_wave_sum(db);
    pn = fx_wave_sum(pn);
    pb = fx_wave_sum(pb);
    if ((threadIdx.x & 63) == 0) {
        if (dn) {
            atomicAdd(sm + SM_KEPT_N, dn);
            atomicAdd(sm + SM_KEPT_B, db);
        }
        if (pn) {
            atomicAdd(sm + SM_Q_N, pn);
            atomicAdd(sm + SM_Q_B, pb);
        }
    }
}

__global__ void __launch_bounds__(FX_THREADS) fqseq_text(FxArgs A)
{
    const int64_t tile = (int64_t)blockIdx.x * FX_TILE;
    const int64_t t_end = (A.nbytes - tile < FX_TILE ? A.nbytes - tile : FX_TILE);
    const int64_t r0 = fx_find(A.out, 0, A.n - 1, A.at + tile);
    const int64_t r1 = fx_find(A.out, r0, A.n - 1, A.at + tile + t_end - 1);
#pragma unroll
    for (int u = 0; u < FX_PER_THREAD; ++u) {
        const int64_t rel = tile + ((int64_t)u * FX_THREADS + threadIdx.x) * 16;
        if (rel >= tile + t_end) break;
        const int m = (int)(A.nbytes - rel < 16 ? A.nbytes - rel : 16);
        const Fx16 v = fx_chunk(A, r0, r1, A.at + rel, m);
        *reinterpret_cast<uint4 *>(A.dst + rel) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
}

}  // namespace

struct cornetto_fqseq {
    cornetto_fqseq_opt_t opt;
    uint8_t *d_win = nullptr;                          // [window + 256]
    uint8_t *d_tail = nullptr;                         // staging of a tail that overlaps its new place
    int64_t tail_cap = 0;
    cornetto_fqrec_t *d_recs = nullptr;                // [rec_cap] the records of the window: what the gets read
    uint32_t *d_size = nullptr, *d_out = nullptr;      // [rec_cap], [rec_cap + 1]
    int64_t rec_cap = 0;
    unsigned long long *d_sm = nullptr;
    // cornetto_fqseq_set_max_err(): the ranges and sums of qmean_sum ([rec_cap] each, allocated with the tables), what passed, the sums kept
    int64_t max_err = -1;
    bool fed = false;
    uint32_t *d_qstart = nullptr, *d_qlen = nullptr;
    unsigned long long *d_qsum = nullptr;
    int64_t qstats[2] = {0, 0};
    std::vector<uint64_t> qsums;
    int64_t carry = 0, text_off = 0;                   // bytes at the front of the window from the last one; the stream offset of the window's first byte
    int64_t n_cur = 0, text_cur = 0;                   // the window the gets read: records with offsets, bytes of text
    int64_t pend_text = -1, pend_end = 0;              // the tail of that window is moved when its gets are through: at the next feed
    int64_t rest = 0;                                  // stream offset of the first byte no record of the device's holds
    int64_t n_rec = 0, n_blocks = 0;
    int64_t stats[4] = {0, 0, 0, 0};
    bool stopped = false;                              // the device's part has ended (plain == 0)
    int64_t err_block = -1;
    std::vector<cornetto_fqrec_t> recs;
    uint8_t *slab[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t slab_cap[4] = {0, 0, 0, 0};
    hipStream_t q[4] = {nullptr, nullptr, nullptr, nullptr};   // kernel + copy of slot s, in order
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // the last copy of slot s
    hipEvent_t tk[4][2] = {};                                  // timing (cornetto_accel_set_timing(2)): around the slot's last kernel
    bool tk_on[4] = {false, false, false, false};
    int64_t tk_bytes[4] = {0, 0, 0, 0};
    double text_ms = 0.0;                                      // fqseq_text in all (cornetto_fqseq_text_time)
    int64_t text_bytes = 0;
    // cornetto_fqseq_get_bgzf(): the slot's packed members on the device, their length (a device word and its pinned copy), where they go
    uint8_t *zpack[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t zpack_cap[4] = {0, 0, 0, 0};
    unsigned long long *d_ztot = nullptr, *p_ztot = nullptr;   // [4]
    hipEvent_t zev[4][2] = {};                                 // the slot's text is written / its members are packed (the handle's stream deflates)
    char *zdst[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t zdst_cap[4] = {0, 0, 0, 0};
    bool zpend[4] = {false, false, false, false};
};

namespace {

// the event pair around the slot's last kernel, once the slot's copy is through
void fx_timed(cornetto_fqseq_t *b, int s)
{
    if (!b->tk_on[s]) return;
    float ms = 0.f;
    if (hipEventSynchronize(b->tk[s][1]) == hipSuccess && hipEventElapsedTime(&ms, b->tk[s][0], b->tk[s][1]) == hipSuccess) {
        b->text_ms += ms;
        b->text_bytes += b->tk_bytes[s];
    }
    b->tk_on[s] = false;
}

// every get of the last window is through; its tail opens the next one
int fx_settle(cornetto_accel_t *h, cornetto_fqseq_t *b)
{
    for (int s = 0; s < 4; ++s) {
        CN_HIP(h, hipEventSynchronize(b->ev[s]));
        fx_timed(b, s);
    }
    b->n_cur = b->text_cur = 0;
    if (b->pend_text < 0) return CORNETTO_OK;
    const int64_t n_text = b->pend_text, end = b->pend_end, carry = n_text - end;
    b->pend_text = -1;
    if (carry > 0 && end > 0) {
        if (carry <= end) {
            CN_HIP(h, hipMemcpyAsync(b->d_win, b->d_win + end, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
        } else {
            if (b->tail_cap < carry) {
                if (b->d_tail) (void)hipFree(b->d_tail);
                b->d_tail = nullptr;
                b->tail_cap = 0;
                if (hipMalloc((void **)&b->d_tail, (size_t)carry) != hipSuccess) {
                    b->d_tail = nullptr;
                    return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: device allocation of %lld bytes failed", (long long)carry);
                }
                b->tail_cap = carry;
            }
            CN_HIP(h, hipMemcpyAsync(b->d_tail, b->d_win + end, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
            CN_HIP(h, hipMemcpyAsync(b->d_win, b->d_tail, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
        }
        CN_HIP(h, hipStreamSynchronize(h->stream));
    }
    b->carry = carry;
    b->text_off += end;
    return CORNETTO_OK;
}

// room for the tables of n records (nothing reads the old ones: the gets are through)
int fx_tables(cornetto_accel_t *h, cornetto_fqseq_t *b, int64_t n)
{
    if (n <= b->rec_cap) return CORNETTO_OK;
    void *old[] = {b->d_recs, b->d_size, b->d_out, b->d_qstart, b->d_qlen, b->d_qsum};
    for (void *p : old)
        if (p) (void)hipFree(p);
    b->d_recs = nullptr;
    b->d_size = b->d_out = b->d_qstart = b->d_qlen = nullptr;
    b->d_qsum = nullptr;
    b->rec_cap = 0;
    const int64_t cap = n + n / 8 + 1024;
    if (hipMalloc((void **)&b->d_recs, (size_t)cap * sizeof(cornetto_fqrec_t)) != hipSuccess || hipMalloc((void **)&b->d_size, (size_t)cap * 4) != hipSuccess ||
        hipMalloc((void **)&b->d_out, ((size_t)cap + 1) * 4) != hipSuccess)
        return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: device allocation of the tables of %lld records failed", (long long)cap);
    if (b->max_err >= 0 && (hipMalloc((void **)&b->d_qstart, (size_t)cap * 4) != hipSuccess || hipMalloc((void **)&b->d_qlen, (size_t)cap * 4) != hipSuccess ||
                            hipMalloc((void **)&b->d_qsum, (size_t)cap * 8) != hipSuccess))
        return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: device allocation of the quality sums of %lld records failed", (long long)cap);
    b->rec_cap = cap;
    return CORNETTO_OK;
}

// the records of window bytes [0, n): index, frame, size, scan; the tail stays where it is until the gets are through
int fx_window(cornetto_accel_t *h, cornetto_fqseq_t *b, int64_t n, bool final, int64_t *n_out)
{
    *n_out = 0;
    b->pend_text = n;
    b->pend_end = 0;
    if (n == 0) return CORNETTO_OK;
    unsigned long long *p_sm = (unsigned long long *)cn_pin(h, PIN_SMALL, 256);
    if (!p_sm) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: pinned allocation failed");
    int last = '\n';
    if (final) CN_TRY(bg_byte_at(h, b->d_win, n - 1, &last));
    cnmarks::Marks mk;
    CN_TRY(cnmarks::count<nl_mask16>(h, "fqseq_feed", "fq_nl_count", "fq_scan", b->d_win, n, WS_FQ_CNT, 0, &mk));
    const int64_t n_nl = mk.total;
    const int64_t n_lines = n_nl + (final && last != '\n' ? 1 : 0);
    const int64_t n_rec = n_lines / 4;
    int64_t n_use = 0, end = 0, text = 0;
    if (n_rec > 0) {
        uint32_t *d_nl = nullptr;
        uint32_t *d_ends = (uint32_t *)cn_ws(h, WS_FQ_ENDS, (size_t)n_rec * 4);
        if (!d_ends) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: workspace allocation failed");
        CN_TRY(fx_tables(h, b, n_rec));
        uint32_t *d_bad = reinterpret_cast<uint32_t *>(b->d_sm + SM_BAD), *d_zero = d_bad + 1;
        CN_HIP(h, hipMemsetAsync(b->d_sm, 0, SM_WORDS * 8, h->stream));
        CN_HIP(h, hipMemsetAsync(b->d_sm + SM_BAD, 0xFF, 8, h->stream));
        CN_TRY(cnmarks::scatter<nl_mask16>(h, "fqseq_feed", "fq_nl_scatter", b->d_win, n, mk, WS_FQ_NL, (size_t)n_nl, &d_nl));
        FqArgs A{b->d_win, n, d_nl, n_nl, n_rec, b->opt.min_len, b->d_recs, d_bad, d_ends};
        CN_LAUNCH(h, "fq_records", fq_records<<<dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, h->stream>>>(A));
        CN_LAUNCH(h, "fqseq_zero", fqseq_zero<<<dim3((unsigned)mk.nt), dim3(cnmarks::MK_THREADS), 0, h->stream>>>(b->d_win, n, d_zero));
        CN_LAUNCH(h, "fqseq_fold", fqseq_fold<<<dim3(1), dim3(64), 0, h->stream>>>(d_zero, d_ends, n_rec, d_bad));
        CN_HIP(h, hipMemcpyAsync(p_sm, b->d_sm + SM_BAD, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        const uint32_t bad = (uint32_t)(p_sm[0] & 0xFFFFFFFFull);
        n_use = (int64_t)bad < n_rec ? (int64_t)bad : n_rec;
        if (n_use < n_rec) b->stopped = true;
        if (n_use > 0) {
            uint32_t *p_end = reinterpret_cast<uint32_t *>(p_sm + 8);
            CN_HIP(h, hipMemcpyAsync(p_end, d_ends + (n_use - 1), 4, hipMemcpyDeviceToHost, h->stream));
            if (b->max_err >= 0) {      // the sums of this window's records alone: the table is zeroed here, whatever it held
                const dim3 grid((unsigned)((n_use + 255) / 256));
                CN_HIP(h, hipMemsetAsync(b->d_qsum, 0, (size_t)n_use * 8, h->stream));
                CN_LAUNCH(h, "fqseq_qrange", fqseq_qrange<<<grid, dim3(256), 0, h->stream>>>(b->d_recs, n_use, b->d_qstart, b->d_qlen));
                CN_TRY(cn_qmean_sum(h, b->d_win, n, b->d_qstart, b->d_qlen, n_use, 0, b->d_qsum));
                CN_LAUNCH(h, "fqseq_qkeep", fqseq_qkeep<<<grid, dim3(256), 0, h->stream>>>(b->d_recs, n_use, b->d_qsum, b->max_err, b->d_sm));
            }
            CN_LAUNCH(h, "fqseq_size", fqseq_size<<<dim3((unsigned)((n_use + 255) / 256)), dim3(256), 0, h->stream>>>(b->d_recs, n_use, b->d_size, b->d_sm));
            CN_TRY(cnscan::exclusive_u32(h, "fqseq_scan", b->d_size, n_use, 1, b->d_out, b->d_sm + SM_TEXT));
            CN_HIP(h, hipMemcpyAsync(b->d_out + n_use, b->d_sm + SM_TEXT, 4, hipMemcpyDeviceToDevice, h->stream));      // out[n]: the text's length (below 2^32)
            CN_HIP(h, hipMemcpyAsync(p_sm + SM_TOTAL_N, b->d_sm + SM_TOTAL_N, (b->max_err >= 0 ? 7 : 5) * 8, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            end = (int64_t)p_end[0];
            text = (int64_t)p_sm[SM_TEXT];
            if (end < 1 || end > n || text < 0 || text > 0xFFFFFFFFll) return cn_fail(h, CORNETTO_E_HIP, "fqseq_feed: a window's text of %lld bytes, its records end at %lld", (long long)text, (long long)end);
            for (int k = 0; k < 4; ++k) b->stats[k] += (int64_t)p_sm[SM_TOTAL_N + k];
            if (b->max_err >= 0) {
                b->qstats[0] += (int64_t)p_sm[SM_Q_N];
                b->qstats[1] += (int64_t)p_sm[SM_Q_B];
            }
            if (b->opt.records && b->max_err >= 0) {
                const size_t at = b->qsums.size();
                b->qsums.resize(at + (size_t)n_use);
                CN_HIP(h, hipMemcpyAsync(b->qsums.data() + at, b->d_qsum, (size_t)n_use * 8, hipMemcpyDeviceToHost, h->stream));
                CN_HIP(h, hipStreamSynchronize(h->stream));
            }
            if (b->opt.records) {
                const size_t at = b->recs.size();
                b->recs.resize(at + (size_t)n_use);
                CN_HIP(h, hipMemcpyAsync(b->recs.data() + at, b->d_recs, (size_t)n_use * sizeof(cornetto_fqrec_t), hipMemcpyDeviceToHost, h->stream));
                CN_HIP(h, hipStreamSynchronize(h->stream));
                for (size_t i = at; i < b->recs.size(); ++i) {      // offsets into the stream, not the window
                    b->recs[i].head += b->text_off;
                    b->recs[i].seq += b->text_off;
                    b->recs[i].qual += b->text_off;
                }
            }
        }
    }
    // at the end of the input whatever follows the last plain record (blank lines, a cut-off record) is the reader's
    if (final && end < n) b->stopped = true;
    b->n_cur = n_use;
    b->text_cur = text;
    b->n_rec += n_use;
    b->pend_end = end;
    b->rest = b->text_off + end;
    *n_out = text;
    return CORNETTO_OK;
}

}  // namespace

extern "C" {

int32_t cornetto_fqseq_tile(void) { return (int32_t)FX_TILE; }

void cornetto_fqseq_defaults(cornetto_fqseq_opt_t *opt)
{
    if (!opt) return;
    opt->min_len = 30000;           // src/seq.c:63
    opt->records = 0;
    opt->window = 256ll << 20;
}

void cornetto_fqseq_close(cornetto_accel_t *h, cornetto_fqseq_t *b)
{
    if (!b) return;
    if (h) (void)hipSetDevice(h->device);
    for (int i = 0; i < 4; ++i)
        if (b->q[i]) { (void)hipStreamSynchronize(b->q[i]); (void)hipStreamDestroy(b->q[i]); }
    for (int i = 0; i < 4; ++i) {
        if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
        if (b->tk[i][0]) (void)hipEventDestroy(b->tk[i][0]);
        if (b->tk[i][1]) (void)hipEventDestroy(b->tk[i][1]);
        if (b->slab[i]) (void)hipFree(b->slab[i]);
        if (b->zpack[i]) (void)hipFree(b->zpack[i]);
        if (b->zev[i][0]) (void)hipEventDestroy(b->zev[i][0]);
        if (b->zev[i][1]) (void)hipEventDestroy(b->zev[i][1]);
    }
    if (b->d_ztot) (void)hipFree(b->d_ztot);
    if (b->p_ztot) (void)hipHostFree(b->p_ztot);
    void *blocks[] = {b->d_win, b->d_tail, b->d_recs, b->d_size, b->d_out, b->d_sm, b->d_qstart, b->d_qlen, b->d_qsum};
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    delete b;
}

int cornetto_fqseq_open(cornetto_accel_t *h, const cornetto_fqseq_opt_t *opt, cornetto_fqseq_t **out)
{
    if (!h || !opt || !out || opt->window < 1 || opt->window > 0xFFFFFF00ll || opt->min_len < 0) return cn_fail(h, CORNETTO_E_ARG, "fqseq_open: bad argument");
    *out = nullptr;
    CN_HIP(h, hipSetDevice(h->device));
    cornetto_fqseq_t *b = new (std::nothrow) cornetto_fqseq;
    if (!b) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_open: host allocation failed");
    b->opt = *opt;
    bool ok = hipMalloc((void **)&b->d_win, (size_t)opt->window + 256) == hipSuccess && hipMalloc((void **)&b->d_sm, SM_WORDS * 8) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipStreamCreateWithFlags(&b->q[i], hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipEventCreateWithFlags(&b->ev[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipEventRecord(b->ev[i], b->q[i]) == hipSuccess;   // (a wait on a slot that has had no get returns at once)
    if (!ok) {
        cornetto_fqseq_close(h, b);
        return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_open: device allocation failed (a window of %lld bytes)", (long long)opt->window);
    }
    *out = b;
    return CORNETTO_OK;
}

int cornetto_fqseq_set_max_err(cornetto_accel_t *h, cornetto_fqseq_t *b, int64_t P)
{
    if (!h || !b || b->fed || P < -1 || P > CORNETTO_QUAL_ONE) return cn_fail(h, CORNETTO_E_ARG, "fqseq_set_max_err: -1 or 0 .. 10^9, before the first feed");
    b->max_err = P;
    return CORNETTO_OK;
}

void cornetto_fqseq_qstats(const cornetto_fqseq_t *b, int64_t *qstats)
{
    if (!b || !qstats) return;
    for (int k = 0; k < 2; ++k) qstats[k] = b->max_err >= 0 ? b->qstats[k] : b->stats[2 + k];
}

int cornetto_fqseq_qsums(cornetto_accel_t *h, cornetto_fqseq_t *b, uint64_t **sums, int64_t *n_sums)
{
    if (!h || !b || !sums || !n_sums) return cn_fail(h, CORNETTO_E_ARG, "fqseq_qsums: bad argument");
    if (!b->opt.records || b->max_err < 0) return cn_fail(h, CORNETTO_E_ARG, "fqseq_qsums: the object keeps no sums (opt.records, cornetto_fqseq_set_max_err)");
    *sums = nullptr;
    *n_sums = (int64_t)b->qsums.size();
    if (b->qsums.empty()) return CORNETTO_OK;
    *sums = (uint64_t *)cn_result_alloc(b->qsums.size() * 8);
    if (!*sums) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_qsums: host allocation failed");
    memcpy(*sums, b->qsums.data(), b->qsums.size() * 8);
    return CORNETTO_OK;
}

int64_t cornetto_fqseq_error(const cornetto_fqseq_t *b) { return b ? b->err_block : -1; }

int64_t cornetto_fqseq_rest(const cornetto_fqseq_t *b) { return b ? b->rest : 0; }

void cornetto_fqseq_stats(const cornetto_fqseq_t *b, int64_t *stats)
{
    if (!b || !stats) return;
    for (int k = 0; k < 4; ++k) stats[k] = b->stats[k];
    stats[4] = b->n_rec;
}

int cornetto_fqseq_feed(cornetto_accel_t *h, cornetto_fqseq_t *b, const cornetto_bgsrc_t *src, int final, int64_t *taken, int64_t *n_text, int32_t *plain)
{
    if (!h || !b || !taken || !n_text || !plain) return cn_fail(h, CORNETTO_E_ARG, "fqseq_feed: bad argument");
    *taken = 0;
    *n_text = 0;
    *plain = b->stopped ? 0 : 1;
    int64_t n_new = 0;
    if (!bgsrc_size(src, &n_new)) return cn_fail(h, CORNETTO_E_ARG, "fqseq_feed: bad source");
    if (b->err_block >= 0) return CORNETTO_E_FORMAT;
    if (b->stopped) return cn_fail(h, CORNETTO_E_ARG, "fqseq_feed: the device's part of the text has ended (cornetto_fqseq_rest)");
    b->fed = true;
    CN_HIP(h, hipSetDevice(h->device));
    CN_TRY(fx_settle(h, b));
    const bool comp = bgsrc_compressed(src);
    const int64_t window = b->opt.window;
    cn_timing_begin(h);
    int64_t bad = -1;
    const int rc = [&]() -> int {
        int64_t n_win = b->carry, got = 0, all = 0;
        if (comp) {
            all = src->n_blocks;
            std::vector<cornetto_bgzf_block_t> grp;
            while (got < all && n_win + src->blocks[got].n_dst <= window) {
                cornetto_bgzf_block_t x = src->blocks[got];
                x.dst = n_win;
                n_win += x.n_dst;
                grp.push_back(x);
                ++got;
            }
            if (got == 0)
                return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: a record of more than %lld bytes does not fit the window of %lld with one more block", (long long)b->carry, (long long)window);
            for (int i = 0; i < 4; ++i) CN_HIP(h, hipStreamSynchronize(src->comp->q[i]));     // every slab is on the device
            CN_TRY(cn_bgzf_inflate_raw(h, src->comp->d, b->d_win, grp.data(), got, &bad));
            if (bad >= 0) n_win = grp[(size_t)bad].dst;        // the records in front of the block first
        } else if (src && src->n > 0) {
            all = src->n;
            got = std::min(all, window - b->carry);
            if (got == 0) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_feed: a record of more than %lld bytes does not fit the window of %lld", (long long)b->carry, (long long)window);
            CN_HIP(h, hipMemcpyAsync(b->d_win + b->carry, src->text, (size_t)got, hipMemcpyHostToDevice, h->stream));
            n_win += got;
        }
        *taken = got;
        const int rw = fx_window(h, b, n_win, final && got == all && bad < 0, n_text);
        CN_HIP(h, hipStreamSynchronize(h->stream));      // (the caller's bytes have left their buffer on every way out)
        return rw;
    }();
    cn_timing_end(h);          // (on every way out of the window: the bracket never stays open)
    *plain = b->stopped ? 0 : 1;
    if (rc != CORNETTO_OK) return rc;
    if (bad >= 0) {
        b->err_block = b->n_blocks + bad;
        return cn_fail(h, CORNETTO_E_FORMAT, "fqseq: BGZF block %lld is not what its footer says", (long long)b->err_block);
    }
    if (comp) b->n_blocks += *taken;
    return CORNETTO_OK;
}

// bytes [at, at + n) of the window's text into the slot's device slab: fqseq_text queued on the slot's queue
static int fx_text_queue(cornetto_accel_t *h, cornetto_fqseq_t *b, int64_t at, int64_t n, int slot)
{
    hipStream_t q = b->q[slot];
    const int64_t need = cn_align_up(n, 16);
    if (b->slab_cap[slot] < need) {              // (the slot's last copy out of the old slab must be through first)
        CN_HIP(h, hipStreamSynchronize(q));
        if (b->slab[slot]) (void)hipFree(b->slab[slot]);
        b->slab[slot] = nullptr;
        b->slab_cap[slot] = 0;
        if (hipMalloc((void **)&b->slab[slot], (size_t)need) != hipSuccess) {
            b->slab[slot] = nullptr;
            return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_get: device slab of %lld bytes", (long long)need);
        }
        b->slab_cap[slot] = need;
    }
    FxArgs A{b->d_win, b->d_recs, b->d_out, b->n_cur, at, n, b->slab[slot]};
    const int64_t blocks = (n + FX_TILE - 1) / FX_TILE;
    if (blocks > INT32_MAX) return cn_fail(h, CORNETTO_E_ARG, "fqseq_get: a range of %lld bytes is too large", (long long)n);
    const bool timed = cn_timed(h, "fqseq_text");
    if (timed) {
        fx_timed(b, slot);
        if (!b->tk[slot][0]) CN_HIP(h, hipEventCreate(&b->tk[slot][0]));
        if (!b->tk[slot][1]) CN_HIP(h, hipEventCreate(&b->tk[slot][1]));
        CN_HIP(h, hipEventRecord(b->tk[slot][0], q));
    }
    fqseq_text<<<dim3((unsigned)blocks), dim3(FX_THREADS), 0, q>>>(A);
    CN_HIP(h, hipGetLastError());
    if (timed) {
        CN_HIP(h, hipEventRecord(b->tk[slot][1], q));
        b->tk_on[slot] = true;
        b->tk_bytes[slot] = n;
    }
    return CORNETTO_OK;
}

int cornetto_fqseq_get(cornetto_accel_t *h, cornetto_fqseq_t *b, char *dst_pinned, int64_t at, int64_t n, int slot)
{
    if (!h || !b || at < 0 || n < 0 || at > b->text_cur - n || slot < 0 || slot > 3 || (n > 0 && !dst_pinned)) return cn_fail(h, CORNETTO_E_ARG, "fqseq_get: bad argument");
    if (n == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    CN_TRY(fx_text_queue(h, b, at, n, slot));
    CN_HIP(h, hipMemcpyAsync(dst_pinned, b->slab[slot], (size_t)n, hipMemcpyDeviceToHost, b->q[slot]));
    CN_HIP(h, hipEventRecord(b->ev[slot], b->q[slot]));
    return CORNETTO_OK;
}

int cornetto_fqseq_get_bgzf(cornetto_accel_t *h, cornetto_fqseq_t *b, char *dst_pinned, int64_t dst_cap, int64_t at, int64_t n, int slot)
{
    if (!h || !b || at < 0 || n < 0 || at > b->text_cur - n || slot < 0 || slot > 3 || dst_cap < 0 || (n > 0 && !dst_pinned))
        return cn_fail(h, CORNETTO_E_ARG, "fqseq_get_bgzf: bad argument");
    const int64_t n_mem = (n + CND_MEMBER - 1) / CND_MEMBER, need = n_mem * CND_STRIDE;
    if (need > dst_cap) return cn_fail(h, CORNETTO_E_ARG, "fqseq_get_bgzf: %lld members want room for %lld bytes, the buffer has %lld", (long long)n_mem, (long long)need, (long long)dst_cap);
    if (n == 0) {
        b->zpend[slot] = false;
        return CORNETTO_OK;
    }
    CN_HIP(h, hipSetDevice(h->device));
    hipStream_t q = b->q[slot];
    if (!b->d_ztot) {
        if (hipMalloc((void **)&b->d_ztot, 4 * 8) != hipSuccess || hipHostMalloc((void **)&b->p_ztot, 4 * 8, hipHostMallocDefault) != hipSuccess)
            return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_get_bgzf: allocation of the length words failed");
    }
    for (int k = 0; k < 2; ++k)
        if (!b->zev[slot][k]) CN_HIP(h, hipEventCreateWithFlags(&b->zev[slot][k], hipEventDisableTiming));
    if (b->zpack_cap[slot] < need) {             // (the slot's last copy out of the old block must be through first)
        CN_HIP(h, hipStreamSynchronize(q));
        if (b->zpack[slot]) (void)hipFree(b->zpack[slot]);
        b->zpack[slot] = nullptr;
        b->zpack_cap[slot] = 0;
        if (hipMalloc((void **)&b->zpack[slot], (size_t)need) != hipSuccess) {
            b->zpack[slot] = nullptr;
            return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_get_bgzf: device block of %lld bytes", (long long)need);
        }
        b->zpack_cap[slot] = need;
    }
    CN_TRY(fx_text_queue(h, b, at, n, slot));
    // the handle's stream deflates behind the slot's text kernel; the slot's queue goes on behind the packed members and their length
    CN_HIP(h, hipEventRecord(b->zev[slot][0], q));
    CN_HIP(h, hipStreamWaitEvent(h->stream, b->zev[slot][0], 0));
    CN_TRY(cn_bgzf_deflate_queue(h, b->slab[slot], n, b->zpack[slot], b->d_ztot + slot));
    CN_HIP(h, hipMemcpyAsync(b->p_ztot + slot, b->d_ztot + slot, 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipEventRecord(b->zev[slot][1], h->stream));
    CN_HIP(h, hipStreamWaitEvent(q, b->zev[slot][1], 0));
    CN_HIP(h, hipEventRecord(b->ev[slot], q));
    b->zdst[slot] = dst_pinned;
    b->zdst_cap[slot] = dst_cap;
    b->zpend[slot] = true;
    return CORNETTO_OK;
}

int cornetto_fqseq_wait_bgzf(cornetto_accel_t *h, cornetto_fqseq_t *b, int slot, int64_t *n_bytes)
{
    if (!h || !b || slot < 0 || slot > 3 || !n_bytes) return cn_fail(h, CORNETTO_E_ARG, "fqseq_wait_bgzf: bad argument");
    *n_bytes = 0;
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipEventSynchronize(b->ev[slot]));
    fx_timed(b, slot);
    if (!b->zpend[slot]) return CORNETTO_OK;
    b->zpend[slot] = false;
    const unsigned long long total = b->p_ztot[slot];
    if (total > (unsigned long long)b->zdst_cap[slot] || total > (unsigned long long)b->zpack_cap[slot])
        return cn_fail(h, CORNETTO_E_HIP, "fqseq_wait_bgzf: %llu bytes of members for a buffer of %lld", total, (long long)b->zdst_cap[slot]);
    if (total) {
        CN_HIP(h, hipMemcpyAsync(b->zdst[slot], b->zpack[slot], (size_t)total, hipMemcpyDeviceToHost, b->q[slot]));
        CN_HIP(h, hipStreamSynchronize(b->q[slot]));
    }
    *n_bytes = (int64_t)total;
    return CORNETTO_OK;
}

int cornetto_fqseq_wait(cornetto_accel_t *h, cornetto_fqseq_t *b, int slot)
{
    if (!h || !b || slot < 0 || slot > 3) return cn_fail(h, CORNETTO_E_ARG, "fqseq_wait: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipEventSynchronize(b->ev[slot]));
    fx_timed(b, slot);
    return CORNETTO_OK;
}

int cornetto_fqseq_text_time(cornetto_accel_t *h, cornetto_fqseq_t *b, double *ms, int64_t *n_bytes)
{
    if (!h || !b || !ms || !n_bytes) return cn_fail(h, CORNETTO_E_ARG, "fqseq_text_time: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    for (int s = 0; s < 4; ++s) {
        CN_HIP(h, hipEventSynchronize(b->ev[s]));
        fx_timed(b, s);
    }
    *ms = b->text_ms;
    *n_bytes = b->text_bytes;
    return CORNETTO_OK;
}

int cornetto_fqseq_records(cornetto_accel_t *h, cornetto_fqseq_t *b, cornetto_fqrec_t **recs, int64_t *n_recs)
{
    if (!h || !b || !recs || !n_recs) return cn_fail(h, CORNETTO_E_ARG, "fqseq_records: bad argument");
    if (!b->opt.records) return cn_fail(h, CORNETTO_E_ARG, "fqseq_records: the object keeps no record table (opt.records)");
    *recs = nullptr;
    *n_recs = (int64_t)b->recs.size();
    if (b->recs.empty()) return CORNETTO_OK;
    *recs = (cornetto_fqrec_t *)cn_result_alloc(b->recs.size() * sizeof(cornetto_fqrec_t));
    if (!*recs) return cn_fail(h, CORNETTO_E_NOMEM, "fqseq_records: host allocation failed");
    memcpy(*recs, b->recs.data(), b->recs.size() * sizeof(cornetto_fqrec_t));
    return CORNETTO_OK;
}

}  // extern "C"
