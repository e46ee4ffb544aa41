// bam.hip — both per-base coverage tracks from a BAM (include/cornetto_accel.h: cornetto_bamdepth_*, cornetto_bam_records).  The caller
// puts the compressed bytes on the device and walks the BGZF chain (cornetto_bgzf_scan); per window of inflated bytes:
//   bgzf_inflate / bgzf_crc32   (inflate.hip) the window's blocks behind the tail the last window left
//   bam_frame     (bamwin.hpp: the window is shared with bamfq.hip) the record chain — block_size, then that many bytes — followed by one
//                 wave (its first lane: every hop is one dependent load): the offsets of the records that lie wholly in the window
//   bam_depth     a wave per record, grid-stride: the checks and the CIGAR walk of bam.hpp, 64 operations per batch, one wave scan of the
//                 reference-advancing lengths per batch; a +1 / -1 pair of integer atomics per run of M = X operations into an int32
//                 difference array per track, laid out like the coverage object (every contig at a multiple of 64 elements): the -1 at a
//                 contig's length lands in the gap behind it, or in element 0 of the next contig, or in the pad — every contig sums to zero
// and at the end
//   bam_scan      one inclusive scan of each difference array (the decoupled look-back of scan.hpp: its uint32 sums are the signed sums
//                 mod 2^32, and every prefix is a depth >= 0), clamped to uint16 with the clamped positions counted: the two arrays
//                 cornetto_cov_wrap() takes.
#include "bam.hpp"
#include "bamwin.hpp"
#include "common.hpp"
#include "scan.hpp"

namespace {

constexpr int BS_THREADS = cnscan::SC_THREADS, BS_ITEMS = 16, BS_TILE = BS_THREADS * BS_ITEMS;
static_assert(BS_TILE == CORNETTO_BAM_SCAN_TILE, "the header publishes the tile size");

struct BamLanes {
    static constexpr int SLOTS = 1;
    __device__ static int first() { return (int)(threadIdx.x & 63); }
    __device__ static int step() { return 64; }
    __device__ static int slot(int) { return 0; }
    __device__ static bool leader() { return (threadIdx.x & 63) == 0; }
    __device__ static void scan(unsigned long long (&v)[1]) { v[0] = cnwave::wave_incl(v[0], (int)(threadIdx.x & 63)); }
    __device__ static unsigned long long last(const unsigned long long (&v)[1]) { return __shfl(v[0], 63); }
    __device__ static unsigned long long sum(const unsigned long long (&v)[1])
    {
        unsigned long long s = v[0];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        return s;
    }
};

struct DiffSink {
    int32_t *tot, *mq;
    __device__ void add(int64_t i, int d, bool q)
    {
        atomicAdd(tot + i, d);
        if (q) atomicAdd(mq + i, d);
    }
};
struct NoSink {
    __device__ void add(int64_t, int, bool) {}
};

// words of the small device block behind the window's own (bamwin.hpp)
enum { SM_ERR = cnbw::BW_ERR, SM_COUNTED = cnbw::BW_OWN, SM_CLAMP = 6, SM_DET = 8, SM_WORDS = cnbw::BW_WORDS };

struct BdArgs {
    const uint8_t *text;
    const uint32_t *off;
    int64_t n_rec, base_rec, text_off;
    CnbRefs R;
    int32_t min_mapq;
    uint32_t skip_flags;
    int32_t *diff[2];          // null: no depth (records only)
    cornetto_bamrec_t *recs;   // null: no record table
    unsigned long long *sm;
};

template <class Sink>
__device__ __forceinline__ int bd_one(const BdArgs &A, int64_t r, Sink &sink, CnbOut &o, CnbErr &e)
{
    return cnb_record<BamLanes>(A.text + A.off[r], A.R, A.min_mapq, A.skip_flags, sink, o, e);
}

__global__ void __launch_bounds__(256) bam_depth(BdArgs A)
{
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    const bool lead = (threadIdx.x & 63) == 0;
    __shared__ unsigned int s_counted;      // the records of the workgroup that count: one atomic per workgroup on the device word
    unsigned int counted = 0;
    if (threadIdx.x == 0) s_counted = 0;
    __syncthreads();
    for (int64_t r = wave; r < A.n_rec; r += n_waves) {
        CnbOut o;
        CnbErr e;
        int kind;
        if (A.diff[0]) {
            DiffSink s{A.diff[0], A.diff[1]};
            kind = bd_one(A, r, s, o, e);
        } else {
            NoSink s;
            kind = bd_one(A, r, s, o, e);
        }
        if (!lead) continue;
        if (kind != CNB_OK) atomicMin(A.sm + SM_ERR, ((unsigned long long)(A.base_rec + r) << 4) | (unsigned)kind);
        else if (o.counted) ++counted;
        if (A.recs) A.recs[r] = cornetto_bamrec_t{A.text_off + (int64_t)A.off[r], o.ref_id, o.pos, o.mapq, o.flag, o.counted, o.n_ops, o.span, o.bases};
    }
    if (lead && counted) atomicAdd(&s_counted, counted);
    __syncthreads();
    if (threadIdx.x == 0 && s_counted) atomicAdd(A.sm + SM_COUNTED, (unsigned long long)s_counted);
}

// the numbers of the record that decided (one wave: the atomicMin above orders the keys, not the detail words)
__global__ void __launch_bounds__(64) bam_detail(BdArgs A, int64_t r)
{
    CnbOut o;
    CnbErr e;
    NoSink s;
    (void)bd_one(A, r, s, o, e);
    if (threadIdx.x == 0) {
        A.sm[SM_DET] = (unsigned long long)(long long)e.a;
        A.sm[SM_DET + 1] = (unsigned long long)(long long)e.b;
    }
}

struct BsArgs {
    const int32_t *diff[2];
    uint16_t *out[2];
    int64_t np;                  // tiles per track: both arrays are np * BS_TILE elements long
    unsigned long long *state;   // [2 np], zeros
    uint32_t *ticket;            // zero
    unsigned long long *n_clamp;
};

__global__ void __launch_bounds__(BS_THREADS) bam_scan(BsArgs A)
{
    __shared__ uint32_t s_gid, s_excl;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) s_gid = atomicAdd(A.ticket, 1u);
    __syncthreads();
    const int64_t gid = s_gid;
    if (gid >= 2 * A.np) return;
    const int q = gid >= A.np ? 1 : 0;
    const int64_t tile = gid - (int64_t)q * A.np;
    const int64_t base = tile * BS_TILE + (int64_t)t * BS_ITEMS;
    uint32_t v[BS_ITEMS], s = 0, bt;
    const int4 *src = reinterpret_cast<const int4 *>(A.diff[q] + base);
#pragma unroll
    for (int k = 0; k < BS_ITEMS / 4; ++k) {
        const int4 x = src[k];
        v[4 * k] = (uint32_t)x.x;
        v[4 * k + 1] = (uint32_t)x.y;
        v[4 * k + 2] = (uint32_t)x.z;
        v[4 * k + 3] = (uint32_t)x.w;
    }
#pragma unroll
    for (int k = 0; k < BS_ITEMS; ++k) s += v[k];
    uint32_t run = cnscan::block_excl<uint32_t, BS_THREADS>(s, bt);
    if (wv == 0) {
        const uint32_t excl = cnscan::lookback_excl(A.state + (int64_t)q * A.np, 1, tile, 1u, bt, lane);
        if (lane == 0) s_excl = excl;
    }
    __syncthreads();
    run += s_excl;
    uint32_t w[BS_ITEMS / 2], n_cl = 0;
#pragma unroll
    for (int k = 0; k < BS_ITEMS; ++k) {
        run += v[k];
        int32_t d = (int32_t)run;
        if (d > 65535) {
            d = 65535;
            ++n_cl;
        }
        if (d < 0) d = 0;          // (no valid file gets here: every prefix is a number of reads)
        if (k & 1) w[k >> 1] |= (uint32_t)d << 16;
        else w[k >> 1] = (uint32_t)d;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(A.out[q] + base);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    n_cl = cnwave::wave_sum(n_cl);
    if (lane == 0 && n_cl) atomicAdd(A.n_clamp, (unsigned long long)n_cl);
}

}  // namespace

struct cornetto_bamdepth {
    cornetto_bamdepth_opt_t opt;
    int32_t n_ref = 0;
    std::vector<int32_t> len;
    std::vector<int64_t> off;          // element offset of contig i (multiple of 64)
    int64_t n_alloc = 0;               // elements of every array: a multiple of the scan tile, 64 and more behind the last contig
    int32_t *d_len = nullptr;
    int64_t *d_off = nullptr;
    int32_t *d_diff[2] = {nullptr, nullptr};
    cnbw::Win w;                       // the window: opt.window bytes, its tail, record offsets and counters
    cornetto_bamrec_t *d_recs = nullptr;
    int64_t n_counted = 0;
    std::vector<cornetto_bamrec_t> recs;
    cornetto_bamerr_t err{0, 0, 0, 0, 0};
    bool finished = false;
};

namespace {

int bam_error(cornetto_accel_t *h, cornetto_bamdepth_t *b, int kind, int64_t record, int64_t a, int64_t c)
{
    b->err = cornetto_bamerr_t{kind, (int32_t)a, (int32_t)c, 0, record};
    return cn_fail(h, CORNETTO_E_FORMAT, "bamdepth: check %d failed at record %lld (%lld, %lld)", kind, (long long)record, (long long)a, (long long)c);
}

BdArgs bd_args(const cornetto_bamdepth_t *b, int64_t n)
{
    BdArgs A{};
    A.text = b->w.win->d;
    A.off = b->w.d_recoff;
    A.n_rec = n;
    A.base_rec = b->w.n_rec;
    A.text_off = b->w.text_off;
    A.R = CnbRefs{b->n_ref, b->d_len, b->d_off};
    A.min_mapq = b->opt.min_mapq;
    A.skip_flags = b->opt.skip_flags;
    A.diff[0] = b->d_diff[0];
    A.diff[1] = b->d_diff[1];
    A.recs = b->d_recs;
    A.sm = b->w.d_sm;
    return A;
}

// the records of window bytes [0, n_text): frame, walk, keep the tail
int bam_window(cornetto_accel_t *h, cornetto_bamdepth_t *b, int64_t n_text)
{
    unsigned long long *p_sm = (unsigned long long *)cn_pin(h, PIN_SMALL, SM_WORDS * 8);
    if (!p_sm) return cn_fail(h, CORNETTO_E_NOMEM, "bamdepth_feed: pinned allocation failed");
    int64_t n = 0, end = 0, ferr_a = 0;
    int ferr = CNB_OK;
    CN_TRY(cnbw::win_frame(h, b->w, "bamdepth_feed", n_text, p_sm, &n, &end, &ferr, &ferr_a));
    BdArgs A = bd_args(b, n);
    if (n > 0) {
        const int64_t blocks = std::min<int64_t>((n + 3) / 4, 16384);
        CN_LAUNCH(h, "bam_depth", bam_depth<<<dim3((unsigned)blocks), dim3(256), 0, h->stream>>>(A));
        CN_HIP(h, hipMemcpyAsync(p_sm + SM_ERR, b->w.d_sm + SM_ERR, 16, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        if (p_sm[SM_ERR] != ~0ull) {
            const int64_t rec = (int64_t)(p_sm[SM_ERR] >> 4);
            CN_LAUNCH(h, "bam_detail", bam_detail<<<dim3(1), dim3(64), 0, h->stream>>>(A, rec - b->w.n_rec));
            CN_HIP(h, hipMemcpyAsync(p_sm + SM_DET, b->w.d_sm + SM_DET, 16, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            return bam_error(h, b, (int)(p_sm[SM_ERR] & 15), rec, (int64_t)p_sm[SM_DET], (int64_t)p_sm[SM_DET + 1]);
        }
        b->n_counted += (int64_t)p_sm[SM_COUNTED];
        if (b->d_recs) {
            const size_t at = b->recs.size();
            b->recs.resize(at + (size_t)n);
            CN_HIP(h, hipMemcpyAsync(b->recs.data() + at, b->d_recs, (size_t)n * sizeof(cornetto_bamrec_t), hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    b->w.n_rec += n;
    if (ferr != CNB_OK) return bam_error(h, b, ferr, b->w.n_rec, ferr_a, 0);
    return cnbw::win_carry(h, b->w, n_text, end);
}

}  // namespace

extern "C" {

int32_t cornetto_bam_scan_tile(void) { return BS_TILE; }

int cornetto_bam_header(const uint8_t *buf, int64_t n, int32_t *n_ref, char ***names, int32_t **lens, int64_t *header_bytes)
{
    if (n < 0 || (n > 0 && !buf) || !n_ref || !names || !lens || !header_bytes) return CORNETTO_E_ARG;
    return cnb_header(buf, n, n_ref, names, lens, header_bytes);
}

void cornetto_bamdepth_defaults(cornetto_bamdepth_opt_t *opt)
{
    if (!opt) return;
    opt->min_mapq = 20;
    opt->skip_flags = 0x704;
    opt->window = 256ll << 20;      // the sweep
    opt->records = 0;
    opt->pad = 0;
}

void cornetto_bamdepth_close(cornetto_accel_t *h, cornetto_bamdepth_t *b)
{
    if (!b) return;
    if (h) (void)hipSetDevice(h->device);
    cnbw::win_close(h, b->w);
    void *blocks[] = {b->d_len, b->d_off, b->d_diff[0], b->d_diff[1], b->d_recs};
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    delete b;
}

int cornetto_bamdepth_open(cornetto_accel_t *h, const cornetto_bamdepth_opt_t *opt, const int32_t *lens, int32_t n_ref, cornetto_bamdepth_t **out)
{
    if (!h || !opt || !out || n_ref < 0 || (n_ref > 0 && !lens) || opt->window < 1 || opt->window > 0xF0000000ll || opt->records < 0 || opt->records > 2)
        return cn_fail(h, CORNETTO_E_ARG, "bamdepth_open: bad argument");
    *out = nullptr;
    CN_HIP(h, hipSetDevice(h->device));
    cornetto_bamdepth_t *b = new (std::nothrow) cornetto_bamdepth;
    if (!b) return cn_fail(h, CORNETTO_E_NOMEM, "bamdepth_open: host allocation failed");
    b->opt = *opt;
    b->n_ref = n_ref;
    int64_t pos = 0;
    for (int32_t i = 0; i < n_ref; ++i) {
        if (lens[i] < 0) {
            delete b;
            return cn_fail(h, CORNETTO_E_ARG, "bamdepth_open: contig %d has a negative length", i);
        }
        b->off.push_back(pos);
        b->len.push_back(lens[i]);
        pos = cn_align_up(pos + lens[i], 64);
    }
    b->n_alloc = cn_align_up(pos + 64, BS_TILE);
    const int rc = [&]() -> int {
        const int ro = cnbw::win_open(h, b->w, opt->window);
        if (ro != CORNETTO_OK && ro != CORNETTO_E_NOMEM) return ro;
        bool ok = ro == CORNETTO_OK && hipMalloc((void **)&b->d_len, (size_t)std::max(n_ref, 1) * 4) == hipSuccess &&
                  hipMalloc((void **)&b->d_off, (size_t)std::max(n_ref, 1) * 8) == hipSuccess;
        if (ok && opt->records) ok = hipMalloc((void **)&b->d_recs, (size_t)b->w.rec_cap * sizeof(cornetto_bamrec_t)) == hipSuccess;
        if (ok && opt->records != 2)
            for (int q = 0; q < 2 && ok; ++q) ok = hipMalloc((void **)&b->d_diff[q], (size_t)b->n_alloc * 4) == hipSuccess;
        if (!ok) return cn_fail(h, CORNETTO_E_NOMEM, "bamdepth_open: device allocation failed (%lld positions)", (long long)b->n_alloc);
        if (n_ref) {
            CN_HIP(h, hipMemcpyAsync(b->d_len, b->len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, h->stream));
            CN_HIP(h, hipMemcpyAsync(b->d_off, b->off.data(), (size_t)n_ref * 8, hipMemcpyHostToDevice, h->stream));
        }
        for (int q = 0; q < 2; ++q)
            if (b->d_diff[q]) CN_HIP(h, hipMemsetAsync(b->d_diff[q], 0, (size_t)b->n_alloc * 4, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        return CORNETTO_OK;
    }();
    if (rc != CORNETTO_OK) {
        cornetto_bamdepth_close(h, b);
        return rc;
    }
    *out = b;
    return CORNETTO_OK;
}

const cornetto_bamerr_t *cornetto_bamdepth_error(const cornetto_bamdepth_t *b) { return b ? &b->err : nullptr; }

int cornetto_bamdepth_feed(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_text_t *comp, const cornetto_bgzf_block_t *blocks, int64_t n_blocks, int64_t skip)
{
    if (!h || !b || !comp || n_blocks < 0 || (n_blocks > 0 && !blocks) || skip < 0) return cn_fail(h, CORNETTO_E_ARG, "bamdepth_feed: bad argument");
    if (b->finished) return cn_fail(h, CORNETTO_E_ARG, "bamdepth_feed: the object is finished");
    if (b->err.kind) return CORNETTO_E_FORMAT;
    if (skip > 0 && (b->w.carry > 0 || b->w.n_rec > 0 || b->w.text_off > 0))
        return cn_fail(h, CORNETTO_E_ARG, "bamdepth_feed: bytes can be skipped only in front of the first record");
    for (int64_t i = 0; i < n_blocks; ++i)
        if (blocks[i].n_dst < 0 || blocks[i].n_dst > 65536) return cn_fail(h, CORNETTO_E_ARG, "bamdepth_feed: block %lld has no BGZF size", (long long)i);
    CN_HIP(h, hipSetDevice(h->device));
    b->w.skip_left += skip;
    std::vector<std::pair<const char *, float>> times;      // (every inflate call opens a timing bracket of its own: the call's kernels are put together here)
    std::vector<cornetto_bgzf_block_t> grp;
    int64_t i = 0;
    while (i < n_blocks) {
        int64_t fill = 0;
        const int64_t j = i + cnbw::win_place(b->w, blocks + i, n_blocks - i, grp, &fill);
        if (j == i) return cn_fail(h, CORNETTO_E_NOMEM, "bamdepth_feed: a record of more than %lld bytes does not fit the window of %lld with one more block",
                                   (long long)b->w.carry, (long long)b->opt.window);
        int64_t bad = -1;
        const int rc = cornetto_text_inflate(h, comp, b->w.win, grp.data(), (int64_t)grp.size(), &bad);
        times.insert(times.end(), h->last.begin(), h->last.end());
        if (rc != CORNETTO_OK && !(rc == CORNETTO_E_FORMAT && bad >= 0)) return rc;
        const int64_t n_text = bad >= 0 ? grp[(size_t)bad].dst : fill;     // a bad block: the records in front of it first
        cn_timing_begin(h);
        const int rw = bam_window(h, b, n_text);
        cn_timing_end(h);          // (on every way out of the window: the bracket never stays open)
        times.insert(times.end(), h->last.begin(), h->last.end());
        h->last = times;
        if (rw != CORNETTO_OK) return rw;
        if (bad >= 0) {
            const int re = bam_error(h, b, CNB_BGZF, b->w.n_rec, b->w.n_blocks + i + bad, 0);
            h->last = times;
            return re;
        }
        i = j;
    }
    b->w.n_blocks += n_blocks;
    return CORNETTO_OK;
}

int cornetto_bamdepth_finish(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_cov_t **cov, int64_t *n_records, int64_t *n_counted, int64_t *n_clamped)
{
    if (!h || !b || !cov) return cn_fail(h, CORNETTO_E_ARG, "bamdepth_finish: bad argument");
    if (b->err.kind) return CORNETTO_E_FORMAT;
    if (b->finished) return cn_fail(h, CORNETTO_E_ARG, "bamdepth_finish: the object is finished");
    *cov = nullptr;
    CN_HIP(h, hipSetDevice(h->device));
    if (b->w.skip_left > 0) return bam_error(h, b, CNB_TRUNC, -1, 0, -1);
    if (b->w.carry > 0) {       // bytes that are no whole record
        uint8_t head[4] = {0, 0, 0, 0};
        if (b->w.carry >= 4) CN_HIP(h, hipMemcpy(head, b->w.win->d, 4, hipMemcpyDeviceToHost));
        return bam_error(h, b, CNB_TRUNC, b->w.n_rec, b->w.carry, b->w.carry >= 4 ? (int64_t)(int32_t)cnb_u32(head) : -1);
    }
    if (n_records) *n_records = b->w.n_rec;
    if (n_counted) *n_counted = b->n_counted;
    if (n_clamped) *n_clamped = 0;
    if (b->opt.records == 2) {
        b->finished = true;
        return CORNETTO_OK;
    }
    const int64_t np = b->n_alloc / BS_TILE;
    if (2 * np > 0x7fffffffll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "bamdepth_finish: more than 2^42 positions");
    uint16_t *d_out[2] = {nullptr, nullptr};
    DevBuf state;
    unsigned long long *p_sm = (unsigned long long *)cn_pin(h, PIN_SMALL, SM_WORDS * 8);
    const bool ok = p_sm && hipMalloc((void **)&d_out[0], (size_t)b->n_alloc * 2) == hipSuccess && hipMalloc((void **)&d_out[1], (size_t)b->n_alloc * 2) == hipSuccess &&
                    state.alloc(64 + (size_t)np * 16) == hipSuccess;
    cn_timing_begin(h);
    const int rc = [&]() -> int {
        if (!ok) return cn_fail(h, CORNETTO_E_NOMEM, "bamdepth_finish: device allocation failed (%lld positions)", (long long)b->n_alloc);
        CN_HIP(h, hipMemsetAsync(state.p, 0, state.bytes, h->stream));
        CN_HIP(h, hipMemsetAsync(b->w.d_sm, 0, SM_WORDS * 8, h->stream));
        BsArgs A{{b->d_diff[0], b->d_diff[1]}, {d_out[0], d_out[1]}, np, reinterpret_cast<unsigned long long *>((uint8_t *)state.p + 64), (uint32_t *)state.p, b->w.d_sm + SM_CLAMP};
        CN_LAUNCH(h, "bam_scan", bam_scan<<<dim3((unsigned)(2 * np)), dim3(BS_THREADS), 0, h->stream>>>(A));
        CN_HIP(h, hipMemcpyAsync(p_sm, b->w.d_sm + SM_CLAMP, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        return CORNETTO_OK;
    }();
    cn_timing_end(h);          // (on every way out: the bracket never stays open)
    cornetto_cov_t *c = nullptr;
    int rw = rc;
    if (rw == CORNETTO_OK) {
        const std::vector<std::pair<const char *, float>> times = h->last;
        rw = cornetto_cov_wrap(h, d_out[0], d_out[1], b->off.data(), b->len.data(), b->n_ref, &c);
        h->last = times;
    }
    if (rw != CORNETTO_OK) {      // (the object is not finished: the difference arrays are whole, the call may be made again)
        if (d_out[0]) (void)hipFree(d_out[0]);
        if (d_out[1]) (void)hipFree(d_out[1]);
        return rw;
    }
    c->owned_d = d_out[0];
    c->owned_q = d_out[1];
    *cov = c;
    b->finished = true;
    if (n_clamped) *n_clamped = (int64_t)p_sm[0];
    for (int q = 0; q < 2; ++q) {      // the difference arrays are no longer needed
        (void)hipFree(b->d_diff[q]);
        b->d_diff[q] = nullptr;
    }
    return CORNETTO_OK;
}

int cornetto_bam_records(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_bamrec_t **recs, int64_t *n_recs)
{
    if (!h || !b || !recs || !n_recs) return cn_fail(h, CORNETTO_E_ARG, "bam_records: bad argument");
    if (!b->opt.records) return cn_fail(h, CORNETTO_E_ARG, "bam_records: the object keeps no record table (opt.records)");
    *recs = nullptr;
    *n_recs = (int64_t)b->recs.size();
    if (b->recs.empty()) return CORNETTO_OK;
    *recs = (cornetto_bamrec_t *)cn_result_alloc(b->recs.size() * sizeof(cornetto_bamrec_t));
    if (!*recs) return cn_fail(h, CORNETTO_E_NOMEM, "bam_records: host allocation failed");
    memcpy(*recs, b->recs.data(), b->recs.size() * sizeof(cornetto_bamrec_t));
    return CORNETTO_OK;
}

}  // extern "C"
