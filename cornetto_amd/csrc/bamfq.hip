// bamfq.hip — the length-filtered FASTQ text of a BAM (include/cornetto_accel.h: cornetto_bamfq_*).  The caller puts the compressed bytes on
// the device and walks the BGZF chain (cornetto_bgzf_scan); per window of inflated bytes (bamwin.hpp: the window, its carried tail and the
// bad-block handling are those of cornetto_bamdepth_feed):
//   bgzf_inflate / bgzf_crc32   (inflate.hip) the window's blocks behind the tail the last window left
//   bam_frame     (bamwin.hpp) the offsets of the records that lie wholly in the window
//   bamfq_size    a thread per record: the checks and the flag, length and dx rules of bamfq.hpp -> the bytes of the record's text (0: not
//                 printed), the counts of the two summary lines (a 64-bit atomic per wave), the error with the lowest record index
//   with cornetto_bamfq_set_max_err() (`seq -q`; nothing of it runs or is allocated otherwise)
//     bamfq_qrange  a thread per record: the quality array of a record that bamfq_size kept as a range of qmean_sum (length 0: not kept, or the
//                   qualities are absent)
//     qmean_sum     (qmean.hip) the sums of quality weights, into a table the window zeroes itself
//     bamfq_qkeep   a thread per record: l_seq * E[1] in place of the sum where the qualities are absent; sum > P * l_seq clears the record's
//                   size and its `kept`; the reads and bases that stay are counted
//   bamfq_scan    the exclusive scan of the sizes (the look-back of scan.hpp): every record's offset in the window's text, and its length
// and per get of bytes [at, at + n) of that text
//   bamfq_text    emit.hip's decomposition: a workgroup writes a tile of consecutive output bytes, a thread 16 bytes with one aligned vector
//                 store (the get starts at slab offset 0).  The tile's records come from a binary search of the offset table, once per tile
//                 (uniform); per chunk a search inside that short range, then cnq_chunk(): 16 bases from 9 source bytes through the nibble
//                 table held in two 64-bit registers, 16 qualities with a SWAR clamp and add, both mirrored for a reverse-strand record, and
//                 every other chunk (header, newlines, a record border, the end of the range) byte by byte into the same two registers.
// or, for cornetto_bamfq_get_bgzf(), behind bamfq_text on the slab
//   bgzf_deflate / bgzf_scan / bgzf_pack   (deflate.hip) the slab's text as BGZF members, packed: only those cross the bus.
// Sizes are 32-bit: a window is at most 2^31 bytes, a record of b bytes prints at most 4 b / 3, so the text of a window is below 2^32.
#include "bamfq.hpp"
#include "bamwin.hpp"
#include "common.hpp"
#include "deflate.hpp"
#include "internal.hpp"
#include "qmean.hpp"
#include "scan.hpp"

namespace {

using namespace cnbw;

constexpr int FQ_THREADS = 256;
constexpr int FQ_PER_THREAD = 4;                                          // 16-byte chunks per thread
constexpr int64_t FQ_TILE = (int64_t)FQ_THREADS * 16 * FQ_PER_THREAD;     // 16 KiB of output per block

// words of the small device block behind the window's own
enum { SM_TOTAL_N = BW_OWN, SM_TOTAL_B = 6, SM_KEPT_N = 7, SM_KEPT_B = 8, SM_TEXT = 9, SM_DET = 10, SM_Q_N = 12, SM_Q_B = 13 };
static_assert(SM_DET + 2 <= SM_Q_N && SM_Q_B < BW_WORDS, "the small block");

struct FsArgs {
    const uint8_t *text;
    const uint32_t *off;
    int64_t n_rec, base_rec, text_off;
    int32_t n_ref, min_len, duplex;
    uint32_t *size;               // [n_rec]
    cornetto_bamfqrec_t *recs;    // null: no record table
    unsigned long long *sm;
};

__device__ __forceinline__ unsigned long long fq_wave_sum(unsigned long long s)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__global__ void __launch_bounds__(256) bamfq_size(FsArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long tn = 0, tb = 0, kn = 0, kb = 0;
    if (r < A.n_rec) {
        CnqOut o;
        CnbErr e;
        const int kind = cnq_size(A.text + A.off[r], A.n_ref, A.min_len, A.duplex, o, e);
        if (kind != CNB_OK) {
            atomicMin(A.sm + BW_ERR, ((unsigned long long)(A.base_rec + r) << 4) | (unsigned)kind);
        } else if (o.kept >= 0) {
            tn = 1;
            tb = (unsigned long long)o.l_seq;
            if (o.kept) {
                kn = 1;
                kb = tb;
            }
        }
        A.size[r] = kind == CNB_OK ? o.size : 0u;
        if (A.recs) A.recs[r] = cornetto_bamfqrec_t{A.text_off + (int64_t)A.off[r], o.l_seq, o.flag, o.name_len, o.kept};
    }
    tn = fq_wave_sum(tn);
    tb = fq_wave_sum(tb);
    kn = fq_wave_sum(kn);
    kb = fq_wave_sum(kb);
    if ((threadIdx.x & 63) == 0 && tn) {
        atomicAdd(A.sm + SM_TOTAL_N, tn);
        atomicAdd(A.sm + SM_TOTAL_B, tb);
        if (kn) {
            atomicAdd(A.sm + SM_KEPT_N, kn);
            atomicAdd(A.sm + SM_KEPT_B, kb);
        }
    }
}

// the numbers of the record that decided (the atomicMin above orders the keys, not the detail words)
__global__ void __launch_bounds__(64) bamfq_detail(FsArgs A, int64_t r)
{
    if (threadIdx.x != 0) return;
    CnqOut o;
    CnbErr e;
    (void)cnq_size(A.text + A.off[r], A.n_ref, A.min_len, A.duplex, o, e);
    A.sm[SM_DET] = (unsigned long long)(long long)e.a;
    A.sm[SM_DET + 1] = (unsigned long long)(long long)e.b;
}

__global__ void __launch_bounds__(256) bamfq_qrange(const uint8_t *__restrict__ text, const uint32_t *__restrict__ off, const uint32_t *__restrict__ size, int64_t n_rec,
                                                    uint32_t *__restrict__ start, uint32_t *__restrict__ len)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    uint32_t s = off[r], l = 0u;         // (a record without text: any place inside it keeps the starts ascending)
    if (size[r]) {                       // (it has passed the checks of cnq_size: its fields lie inside it)
        const CnqRec x = cnq_rec(text + off[r]);
        s = (uint32_t)(x.qual - text);
        l = x.no_qual ? 0u : (uint32_t)x.S;
    }
    start[r] = s;
    len[r] = l;
}

__global__ void __launch_bounds__(256) bamfq_qkeep(const uint8_t *__restrict__ text, const uint32_t *__restrict__ off, uint32_t *__restrict__ size, int64_t n_rec,
                                                   unsigned long long *__restrict__ sum, int64_t max_err, cornetto_bamfqrec_t *recs, unsigned long long *sm)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long pn = 0, pb = 0;
    if (r < n_rec && size[r]) {
        const CnqRec x = cnq_rec(text + off[r]);
        const unsigned long long L = (unsigned long long)x.S;
        unsigned long long s = sum[r];
        if (x.no_qual) sum[r] = s = L * qm_e(1);      // every quality prints as '"'
        if (s > (unsigned long long)max_err * L) {
            size[r] = 0u;
            if (recs) recs[r].kept = 0;
        } else {
            pn = 1;
            pb = L;
        }
    }
    pn = fq_wave_sum(pn);
    pb = fq_wave_sum(pb);
    if ((threadIdx.x & 63) == 0 && pn) {
        atomicAdd(sm + SM_Q_N, pn);
        atomicAdd(sm + SM_Q_B, pb);
    }
}

struct FtArgs {
    CnqSrc S;
    int64_t at, nbytes;
    uint8_t *dst;      // at least nbytes rounded up to 16
};

__global__ void __launch_bounds__(FQ_THREADS) bamfq_text(FtArgs A)
{
    const int64_t tile = (int64_t)blockIdx.x * FQ_TILE;
    const int64_t t_end = (A.nbytes - tile < FQ_TILE ? A.nbytes - tile : FQ_TILE);
    const int64_t r0 = cnq_find(A.S.out, 0, A.S.n - 1, A.at + tile);
    const int64_t r1 = cnq_find(A.S.out, r0, A.S.n - 1, A.at + tile + t_end - 1);
#pragma unroll
    for (int u = 0; u < FQ_PER_THREAD; ++u) {
        const int64_t rel = tile + ((int64_t)u * FQ_THREADS + threadIdx.x) * 16;
        if (rel >= tile + t_end) break;
        const int m = (int)(A.nbytes - rel < 16 ? A.nbytes - rel : 16);
        uint64_t v[2];
        cnq_chunk(A.S, r0, r1, A.at + rel, m, v);
        *reinterpret_cast<uint4 *>(A.dst + rel) = make_uint4((uint32_t)v[0], (uint32_t)(v[0] >> 32), (uint32_t)v[1], (uint32_t)(v[1] >> 32));
    }
}

}  // namespace

struct cornetto_bamfq {
    cornetto_bamfq_opt_t opt;
    cnbw::Win w;
    uint32_t *d_size = nullptr, *d_out = nullptr;      // [rec_cap], [rec_cap + 1]
    cornetto_bamfqrec_t *d_recs = nullptr;
    int64_t n_cur = 0, text_cur = 0;                   // the window the gets read: records with offsets, bytes of text
    int64_t pend_text = -1, pend_end = 0;              // the tail of that window is moved when its gets are through: at the next feed
    int64_t stats[4] = {0, 0, 0, 0};
    std::vector<cornetto_bamfqrec_t> recs;
    cornetto_bamerr_t err{0, 0, 0, 0, 0};
    // cornetto_bamfq_set_max_err(): the ranges and sums of qmean_sum ([q_cap] each, grown by the window that needs them), what passed, the sums kept
    int64_t max_err = -1;
    bool fed = false;
    uint32_t *d_qstart = nullptr, *d_qlen = nullptr;
    unsigned long long *d_qsum = nullptr;
    int64_t q_cap = 0;
    int64_t qstats[2] = {0, 0};
    std::vector<uint64_t> qsums;
    uint8_t *slab[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t slab_cap[4] = {0, 0, 0, 0};
    hipStream_t q[4] = {nullptr, nullptr, nullptr, nullptr};   // kernel + copy of slot s, in order
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // the last copy of slot s
    hipEvent_t tk[4][2] = {};                                  // timing (cornetto_accel_set_timing(2)): around the slot's last kernel
    bool tk_on[4] = {false, false, false, false};
    float text_ms = 0.f;                                       // bamfq_text in all: handed to cornetto_accel_last_timing() by the finish
    int64_t text_n = 0;
    // cornetto_bamfq_get_bgzf(): the slot's packed members on the device, their length (a device word and its pinned copy), where they go
    uint8_t *zpack[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t zpack_cap[4] = {0, 0, 0, 0};
    unsigned long long *d_ztot = nullptr, *p_ztot = nullptr;   // [4]
    hipEvent_t zev[4][2] = {};                                 // the slot's text is written / its members are packed (the handle's stream deflates)
    char *zdst[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t zdst_cap[4] = {0, 0, 0, 0};
    bool zpend[4] = {false, false, false, false};
};

namespace {

int fq_error(cornetto_accel_t *h, cornetto_bamfq_t *b, int kind, int64_t record, int64_t a, int64_t c)
{
    b->err = cornetto_bamerr_t{kind, (int32_t)a, (int32_t)c, 0, record};
    return cn_fail(h, CORNETTO_E_FORMAT, "bamfq: check %d failed at record %lld (%lld, %lld)", kind, (long long)record, (long long)a, (long long)c);
}

// the event pair around the slot's last kernel, once the slot's copy is through
void fq_timed(cornetto_bamfq_t *b, int s)
{
    if (!b->tk_on[s]) return;
    float ms = 0.f;
    if (hipEventSynchronize(b->tk[s][1]) == hipSuccess && hipEventElapsedTime(&ms, b->tk[s][0], b->tk[s][1]) == hipSuccess) {
        b->text_ms += ms;
        ++b->text_n;
    }
    b->tk_on[s] = false;
}

// every get of the last window is through; its tail opens the next one
int fq_settle(cornetto_accel_t *h, cornetto_bamfq_t *b)
{
    for (int s = 0; s < 4; ++s) {
        CN_HIP(h, hipEventSynchronize(b->ev[s]));
        fq_timed(b, s);
    }
    b->n_cur = b->text_cur = 0;
    if (b->pend_text >= 0) {
        const int64_t n_text = b->pend_text;
        b->pend_text = -1;
        CN_TRY(win_carry(h, b->w, n_text, b->pend_end));
    }
    return CORNETTO_OK;
}

FsArgs fs_args(const cornetto_bamfq_t *b, int64_t n)
{
    FsArgs A{};
    A.text = b->w.win->d;
    A.off = b->w.d_recoff;
    A.n_rec = n;
    A.base_rec = b->w.n_rec;
    A.text_off = b->w.text_off;
    A.n_ref = b->opt.n_ref;
    A.min_len = b->opt.min_len;
    A.duplex = b->opt.duplex;
    A.size = b->d_size;
    A.recs = b->d_recs;
    A.sm = b->w.d_sm;
    return A;
}

int fq_launch_size(cornetto_accel_t *h, const FsArgs &A)
{
    CN_LAUNCH(h, "bamfq_size", bamfq_size<<<dim3((unsigned)((A.n_rec + 255) / 256)), dim3(256), 0, h->stream>>>(A));
    return CORNETTO_OK;
}

// `seq -q` for the window's first n records, between their sizes and the scan: the sums of this window's records alone (the table is zeroed
// here, whatever it held), then the decision
int fq_qmean(cornetto_accel_t *h, cornetto_bamfq_t *b, int64_t n, int64_t n_text)
{
    if (n > b->q_cap) {
        void *old[] = {b->d_qstart, b->d_qlen, b->d_qsum};
        for (void *p : old)
            if (p) (void)hipFree(p);
        b->d_qstart = b->d_qlen = nullptr;
        b->d_qsum = nullptr;
        b->q_cap = 0;
        const int64_t cap = std::min(n + n / 8 + 1024, b->w.rec_cap);
        if (hipMalloc((void **)&b->d_qstart, (size_t)cap * 4) != hipSuccess || hipMalloc((void **)&b->d_qlen, (size_t)cap * 4) != hipSuccess ||
            hipMalloc((void **)&b->d_qsum, (size_t)cap * 8) != hipSuccess)
            return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_feed: device allocation of the quality sums of %lld records failed", (long long)cap);
        b->q_cap = cap;
    }
    const dim3 grid((unsigned)((n + 255) / 256));
    const uint8_t *text = b->w.win->d;
    CN_HIP(h, hipMemsetAsync(b->d_qsum, 0, (size_t)n * 8, h->stream));
    CN_HIP(h, hipMemsetAsync(b->w.d_sm + SM_Q_N, 0, 2 * 8, h->stream));
    CN_LAUNCH(h, "bamfq_qrange", bamfq_qrange<<<grid, dim3(256), 0, h->stream>>>(text, b->w.d_recoff, b->d_size, n, b->d_qstart, b->d_qlen));
    CN_TRY(cn_qmean_sum(h, text, n_text, b->d_qstart, b->d_qlen, n, 1, b->d_qsum));
    CN_LAUNCH(h, "bamfq_qkeep", bamfq_qkeep<<<grid, dim3(256), 0, h->stream>>>(text, b->w.d_recoff, b->d_size, n, b->d_qsum, b->max_err, b->d_recs, b->w.d_sm));
    return CORNETTO_OK;
}

// the records of window bytes [0, n_text): frame, size, scan; the tail stays where it is until the gets are through
int fq_window(cornetto_accel_t *h, cornetto_bamfq_t *b, int64_t n_text, int64_t *n_out)
{
    unsigned long long *p_sm = (unsigned long long *)cn_pin(h, PIN_SMALL, BW_WORDS * 8);
    if (!p_sm) return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_feed: pinned allocation failed");
    int64_t n = 0, end = 0, ferr_a = 0;
    int ferr = CNB_OK;
    CN_TRY(win_frame(h, b->w, "bamfq_feed", n_text, p_sm, &n, &end, &ferr, &ferr_a));
    int64_t n_ok = n;              // records in front of the first one that fails a check
    int bad_kind = CNB_OK;
    int64_t det[2] = {0, 0};
    if (n > 0) {
        FsArgs A = fs_args(b, n);
        CN_TRY(fq_launch_size(h, A));
        CN_HIP(h, hipMemcpyAsync(p_sm + BW_ERR, b->w.d_sm + BW_ERR, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        if (p_sm[BW_ERR] != ~0ull) {
            const int64_t rec = (int64_t)(p_sm[BW_ERR] >> 4) - b->w.n_rec;
            if (rec < 0 || rec >= n) return cn_fail(h, CORNETTO_E_HIP, "bamfq_feed: an error outside the window's records");
            bad_kind = (int)(p_sm[BW_ERR] & 15);
            CN_LAUNCH(h, "bamfq_detail", bamfq_detail<<<dim3(1), dim3(64), 0, h->stream>>>(A, rec));
            CN_HIP(h, hipMemcpyAsync(p_sm + SM_DET, b->w.d_sm + SM_DET, 16, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            det[0] = (int64_t)p_sm[SM_DET];
            det[1] = (int64_t)p_sm[SM_DET + 1];
            n_ok = rec;
            // the counts of the records in front of it alone: the pass again over those (a file that fails does so once)
            CN_HIP(h, hipMemsetAsync(b->w.d_sm + SM_TOTAL_N, 0, 4 * 8, h->stream));
            if (n_ok > 0) CN_TRY(fq_launch_size(h, fs_args(b, n_ok)));
        }
    }
    int64_t text = 0;
    if (n_ok > 0) {
        if (b->max_err >= 0) CN_TRY(fq_qmean(h, b, n_ok, n_text));
        CN_TRY(cnscan::exclusive_u32(h, "bamfq_scan", b->d_size, n_ok, 1, b->d_out, b->w.d_sm + SM_TEXT));
        CN_HIP(h, hipMemcpyAsync(b->d_out + n_ok, b->w.d_sm + SM_TEXT, 4, hipMemcpyDeviceToDevice, h->stream));      // out[n]: the text's length (below 2^32)
        CN_HIP(h, hipMemcpyAsync(p_sm + SM_TOTAL_N, b->w.d_sm + SM_TOTAL_N, 5 * 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        text = (int64_t)p_sm[SM_TEXT];
        if (text < 0 || text > 0xFFFFFFFFll) return cn_fail(h, CORNETTO_E_HIP, "bamfq_feed: a window's text of %lld bytes", (long long)text);
        for (int k = 0; k < 4; ++k) b->stats[k] += (int64_t)p_sm[SM_TOTAL_N + k];
        if (b->max_err >= 0) {
            CN_HIP(h, hipMemcpyAsync(p_sm + SM_Q_N, b->w.d_sm + SM_Q_N, 2 * 8, hipMemcpyDeviceToHost, h->stream));
            if (b->d_recs) {
                const size_t at = b->qsums.size();
                b->qsums.resize(at + (size_t)n_ok);
                CN_HIP(h, hipMemcpyAsync(b->qsums.data() + at, b->d_qsum, (size_t)n_ok * 8, hipMemcpyDeviceToHost, h->stream));
            }
            CN_HIP(h, hipStreamSynchronize(h->stream));
            b->qstats[0] += (int64_t)p_sm[SM_Q_N];
            b->qstats[1] += (int64_t)p_sm[SM_Q_B];
        }
        if (b->d_recs) {
            const size_t at = b->recs.size();
            b->recs.resize(at + (size_t)n_ok);
            CN_HIP(h, hipMemcpyAsync(b->recs.data() + at, b->d_recs, (size_t)n_ok * sizeof(cornetto_bamfqrec_t), hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    b->n_cur = n_ok;
    b->text_cur = text;
    *n_out = text;
    b->pend_text = n_text;
    b->pend_end = end;
    if (bad_kind != CNB_OK) {
        const int64_t rec = b->w.n_rec + n_ok;
        b->w.n_rec = rec;
        return fq_error(h, b, bad_kind, rec, det[0], det[1]);
    }
    b->w.n_rec += n;
    if (ferr != CNB_OK) return fq_error(h, b, ferr, b->w.n_rec, ferr_a, 0);
    return CORNETTO_OK;
}

}  // namespace

extern "C" {

void cornetto_bamfq_defaults(cornetto_bamfq_opt_t *opt)
{
    if (!opt) return;
    opt->min_len = 30000;           // src/seq.c:63
    opt->duplex = 0;
    opt->window = 256ll << 20;      // the sweep of the depth reader's window
    opt->n_ref = 0;
    opt->records = 0;
}

void cornetto_bamfq_close(cornetto_accel_t *h, cornetto_bamfq_t *b)
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
    cnbw::win_close(h, b->w);
    void *blocks[] = {b->d_size, b->d_out, b->d_recs, b->d_qstart, b->d_qlen, b->d_qsum};
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    delete b;
}

int cornetto_bamfq_open(cornetto_accel_t *h, const cornetto_bamfq_opt_t *opt, cornetto_bamfq_t **out)
{
    if (!h || !opt || !out || opt->window < 1 || opt->window > 0x80000000ll || opt->min_len < 0 || opt->n_ref < 0) return cn_fail(h, CORNETTO_E_ARG, "bamfq_open: bad argument");
    *out = nullptr;
    CN_HIP(h, hipSetDevice(h->device));
    cornetto_bamfq_t *b = new (std::nothrow) cornetto_bamfq;
    if (!b) return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_open: host allocation failed");
    b->opt = *opt;
    const int rc = [&]() -> int {
        const int ro = cnbw::win_open(h, b->w, opt->window);
        if (ro != CORNETTO_OK && ro != CORNETTO_E_NOMEM) return ro;
        bool ok = ro == CORNETTO_OK && hipMalloc((void **)&b->d_size, (size_t)b->w.rec_cap * 4) == hipSuccess &&
                  hipMalloc((void **)&b->d_out, ((size_t)b->w.rec_cap + 1) * 4) == hipSuccess;
        if (ok && opt->records) ok = hipMalloc((void **)&b->d_recs, (size_t)b->w.rec_cap * sizeof(cornetto_bamfqrec_t)) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipStreamCreateWithFlags(&b->q[i], hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventCreateWithFlags(&b->ev[i], hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventRecord(b->ev[i], b->q[i]) == hipSuccess;   // (a wait on a slot that has had no get returns at once)
        if (!ok) return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_open: device allocation failed (a window of %lld bytes)", (long long)opt->window);
        return CORNETTO_OK;
    }();
    if (rc != CORNETTO_OK) {
        cornetto_bamfq_close(h, b);
        return rc;
    }
    *out = b;
    return CORNETTO_OK;
}

const cornetto_bamerr_t *cornetto_bamfq_error(const cornetto_bamfq_t *b) { return b ? &b->err : nullptr; }

int cornetto_bamfq_set_max_err(cornetto_accel_t *h, cornetto_bamfq_t *b, int64_t P)
{
    if (!h || !b || b->fed || P < -1 || P > CORNETTO_QUAL_ONE) return cn_fail(h, CORNETTO_E_ARG, "bamfq_set_max_err: -1 or 0 .. 10^9, before the first feed");
    b->max_err = P;
    return CORNETTO_OK;
}

void cornetto_bamfq_qstats(const cornetto_bamfq_t *b, int64_t *qstats)
{
    if (!b || !qstats) return;
    for (int k = 0; k < 2; ++k) qstats[k] = b->max_err >= 0 ? b->qstats[k] : b->stats[2 + k];
}

int cornetto_bamfq_qsums(cornetto_accel_t *h, cornetto_bamfq_t *b, uint64_t **sums, int64_t *n_sums)
{
    if (!h || !b || !sums || !n_sums) return cn_fail(h, CORNETTO_E_ARG, "bamfq_qsums: bad argument");
    if (!b->opt.records || b->max_err < 0) return cn_fail(h, CORNETTO_E_ARG, "bamfq_qsums: the object keeps no sums (opt.records, cornetto_bamfq_set_max_err)");
    *sums = nullptr;
    *n_sums = (int64_t)b->qsums.size();
    if (b->qsums.empty()) return CORNETTO_OK;
    *sums = (uint64_t *)cn_result_alloc(b->qsums.size() * 8);
    if (!*sums) return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_qsums: host allocation failed");
    memcpy(*sums, b->qsums.data(), b->qsums.size() * 8);
    return CORNETTO_OK;
}

void cornetto_bamfq_stats(const cornetto_bamfq_t *b, int64_t *stats)
{
    if (!b || !stats) return;
    for (int k = 0; k < 4; ++k) stats[k] = b->stats[k];
    stats[4] = b->w.n_rec;
}

int cornetto_bamfq_feed(cornetto_accel_t *h, cornetto_bamfq_t *b, cornetto_text_t *comp, const cornetto_bgzf_block_t *blocks, int64_t n_blocks, int64_t skip,
                        int64_t *taken, int64_t *n_text)
{
    if (!h || !b || !comp || !taken || !n_text || n_blocks < 0 || (n_blocks > 0 && !blocks) || skip < 0) return cn_fail(h, CORNETTO_E_ARG, "bamfq_feed: bad argument");
    *taken = 0;
    *n_text = 0;
    if (b->err.kind) return CORNETTO_E_FORMAT;
    b->fed = true;
    for (int64_t i = 0; i < n_blocks; ++i)
        if (blocks[i].n_dst < 0 || blocks[i].n_dst > 65536) return cn_fail(h, CORNETTO_E_ARG, "bamfq_feed: block %lld has no BGZF size", (long long)i);
    CN_HIP(h, hipSetDevice(h->device));
    CN_TRY(fq_settle(h, b));
    if (skip > 0 && (b->w.carry > 0 || b->w.n_rec > 0 || b->w.text_off > 0))
        return cn_fail(h, CORNETTO_E_ARG, "bamfq_feed: bytes can be skipped only in front of the first record");
    b->w.skip_left += skip;
    if (n_blocks == 0) return CORNETTO_OK;
    std::vector<cornetto_bgzf_block_t> grp;
    int64_t fill = 0;
    const int64_t j = cnbw::win_place(b->w, blocks, n_blocks, grp, &fill);
    if (j == 0) {
        b->w.skip_left -= skip;       // (nothing was taken: the call may be made again on another path)
        return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_feed: a record of more than %lld bytes does not fit the window of %lld with one more block", (long long)b->w.carry,
                       (long long)b->opt.window);
    }
    int64_t bad = -1;
    const int rc = cornetto_text_inflate(h, comp, b->w.win, grp.data(), (int64_t)grp.size(), &bad);
    std::vector<std::pair<const char *, float>> times = h->last;      // (the inflate call opens a timing bracket of its own: the feed's kernels are put together)
    if (rc != CORNETTO_OK && !(rc == CORNETTO_E_FORMAT && bad >= 0)) return rc;
    const int64_t n_win = bad >= 0 ? grp[(size_t)bad].dst : fill;     // a bad block: the records in front of it first
    cn_timing_begin(h);
    const int rw = fq_window(h, b, n_win, n_text);
    cn_timing_end(h);          // (on every way out of the window: the bracket never stays open)
    times.insert(times.end(), h->last.begin(), h->last.end());
    h->last = times;
    *taken = j;
    if (rw != CORNETTO_OK) return rw;
    if (bad >= 0) {
        const int re = fq_error(h, b, CNB_BGZF, b->w.n_rec, b->w.n_blocks + bad, 0);
        h->last = times;
        return re;
    }
    b->w.n_blocks += j;
    return CORNETTO_OK;
}

int cornetto_bamfq_finish(cornetto_accel_t *h, cornetto_bamfq_t *b)
{
    if (!h || !b) return cn_fail(h, CORNETTO_E_ARG, "bamfq_finish: bad argument");
    if (b->err.kind) return CORNETTO_E_FORMAT;
    CN_HIP(h, hipSetDevice(h->device));
    CN_TRY(fq_settle(h, b));
    h->last.clear();
    if (b->text_n) h->last.emplace_back("bamfq_text", b->text_ms);      // (the gets run on the slots' queues, outside every bracket of the handle's stream)
    if (b->w.skip_left > 0) return fq_error(h, b, CNB_TRUNC, -1, 0, -1);
    if (b->w.carry > 0) {       // bytes that are no whole record
        uint8_t head[4] = {0, 0, 0, 0};
        if (b->w.carry >= 4) CN_HIP(h, hipMemcpy(head, b->w.win->d, 4, hipMemcpyDeviceToHost));
        return fq_error(h, b, CNB_TRUNC, b->w.n_rec, b->w.carry, b->w.carry >= 4 ? (int64_t)(int32_t)cnb_u32(head) : -1);
    }
    return CORNETTO_OK;
}

// bytes [at, at + n) of the window's text into the slot's device slab: bamfq_text queued on the slot's queue
static int fq_text_queue(cornetto_accel_t *h, cornetto_bamfq_t *b, int64_t at, int64_t n, int slot)
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
            return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_get: device slab of %lld bytes", (long long)need);
        }
        b->slab_cap[slot] = need;
    }
    FtArgs A{CnqSrc{b->w.win->d, b->w.d_recoff, b->d_out, b->n_cur}, at, n, b->slab[slot]};
    const int64_t blocks = (n + FQ_TILE - 1) / FQ_TILE;
    if (blocks > INT32_MAX) return cn_fail(h, CORNETTO_E_ARG, "bamfq_get: a range of %lld bytes is too large", (long long)n);
    const bool timed = cn_timed(h, "bamfq_text");
    if (timed) {
        fq_timed(b, slot);
        if (!b->tk[slot][0]) CN_HIP(h, hipEventCreate(&b->tk[slot][0]));
        if (!b->tk[slot][1]) CN_HIP(h, hipEventCreate(&b->tk[slot][1]));
        CN_HIP(h, hipEventRecord(b->tk[slot][0], q));
    }
    bamfq_text<<<dim3((unsigned)blocks), dim3(FQ_THREADS), 0, q>>>(A);
    CN_HIP(h, hipGetLastError());
    if (timed) {
        CN_HIP(h, hipEventRecord(b->tk[slot][1], q));
        b->tk_on[slot] = true;
    }
    return CORNETTO_OK;
}

int cornetto_bamfq_get(cornetto_accel_t *h, cornetto_bamfq_t *b, char *dst_pinned, int64_t at, int64_t n, int slot)
{
    if (!h || !b || at < 0 || n < 0 || at > b->text_cur - n || slot < 0 || slot > 3 || (n > 0 && !dst_pinned)) return cn_fail(h, CORNETTO_E_ARG, "bamfq_get: bad argument");
    if (n == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    CN_TRY(fq_text_queue(h, b, at, n, slot));
    CN_HIP(h, hipMemcpyAsync(dst_pinned, b->slab[slot], (size_t)n, hipMemcpyDeviceToHost, b->q[slot]));
    CN_HIP(h, hipEventRecord(b->ev[slot], b->q[slot]));
    return CORNETTO_OK;
}

int cornetto_bamfq_get_bgzf(cornetto_accel_t *h, cornetto_bamfq_t *b, char *dst_pinned, int64_t dst_cap, int64_t at, int64_t n, int slot)
{
    if (!h || !b || at < 0 || n < 0 || at > b->text_cur - n || slot < 0 || slot > 3 || dst_cap < 0 || (n > 0 && !dst_pinned))
        return cn_fail(h, CORNETTO_E_ARG, "bamfq_get_bgzf: bad argument");
    const int64_t n_mem = (n + CND_MEMBER - 1) / CND_MEMBER, need = n_mem * CND_STRIDE;
    if (need > dst_cap) return cn_fail(h, CORNETTO_E_ARG, "bamfq_get_bgzf: %lld members want room for %lld bytes, the buffer has %lld", (long long)n_mem, (long long)need, (long long)dst_cap);
    if (n == 0) {
        b->zpend[slot] = false;
        return CORNETTO_OK;
    }
    CN_HIP(h, hipSetDevice(h->device));
    hipStream_t q = b->q[slot];
    if (!b->d_ztot) {
        if (hipMalloc((void **)&b->d_ztot, 4 * 8) != hipSuccess || hipHostMalloc((void **)&b->p_ztot, 4 * 8, hipHostMallocDefault) != hipSuccess)
            return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_get_bgzf: allocation of the length words failed");
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
            return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_get_bgzf: device block of %lld bytes", (long long)need);
        }
        b->zpack_cap[slot] = need;
    }
    CN_TRY(fq_text_queue(h, b, at, n, slot));
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

int cornetto_bamfq_wait_bgzf(cornetto_accel_t *h, cornetto_bamfq_t *b, int slot, int64_t *n_bytes)
{
    if (!h || !b || slot < 0 || slot > 3 || !n_bytes) return cn_fail(h, CORNETTO_E_ARG, "bamfq_wait_bgzf: bad argument");
    *n_bytes = 0;
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipEventSynchronize(b->ev[slot]));
    fq_timed(b, slot);
    if (!b->zpend[slot]) return CORNETTO_OK;
    b->zpend[slot] = false;
    const unsigned long long total = b->p_ztot[slot];
    if (total > (unsigned long long)b->zdst_cap[slot] || total > (unsigned long long)b->zpack_cap[slot])
        return cn_fail(h, CORNETTO_E_HIP, "bamfq_wait_bgzf: %llu bytes of members for a buffer of %lld", total, (long long)b->zdst_cap[slot]);
    if (total) {
        CN_HIP(h, hipMemcpyAsync(b->zdst[slot], b->zpack[slot], (size_t)total, hipMemcpyDeviceToHost, b->q[slot]));
        CN_HIP(h, hipStreamSynchronize(b->q[slot]));
    }
    *n_bytes = (int64_t)total;
    return CORNETTO_OK;
}

int cornetto_bamfq_wait(cornetto_accel_t *h, cornetto_bamfq_t *b, int slot)
{
    if (!h || !b || slot < 0 || slot > 3) return cn_fail(h, CORNETTO_E_ARG, "bamfq_wait: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipEventSynchronize(b->ev[slot]));
    fq_timed(b, slot);
    return CORNETTO_OK;
}

int cornetto_bamfq_records(cornetto_accel_t *h, cornetto_bamfq_t *b, cornetto_bamfqrec_t **recs, int64_t *n_recs)
{
    if (!h || !b || !recs || !n_recs) return cn_fail(h, CORNETTO_E_ARG, "bamfq_records: bad argument");
    if (!b->opt.records) return cn_fail(h, CORNETTO_E_ARG, "bamfq_records: the object keeps no record table (opt.records)");
    *recs = nullptr;
    *n_recs = (int64_t)b->recs.size();
    if (b->recs.empty()) return CORNETTO_OK;
    *recs = (cornetto_bamfqrec_t *)cn_result_alloc(b->recs.size() * sizeof(cornetto_bamfqrec_t));
    if (!*recs) return cn_fail(h, CORNETTO_E_NOMEM, "bamfq_records: host allocation failed");
    memcpy(*recs, b->recs.data(), b->recs.size() * sizeof(cornetto_bamfqrec_t));
    return CORNETTO_OK;
}

}  // extern "C"
