// bgrun.hip — device ingest of two RUN-LENGTH bedgraphs (`name start end value`, one record per run of equal depth: mosdepth per-base
// output, bedtools genomecov -bga) for `(no)boringbits --runs`.  An extension: the reference reads one line per base only (bgin.hip).  The
// result is defined by expansion — every record `name s e v` stands for the per-base records `name p p+1 v`, p = s .. e-1 — and is the same
// cornetto_cov_t the per-base reader makes.
//
// The two files are independent streams (their run boundaries differ).  Per feed of one file:
//   tk_count / tk_scatter   token starts (bgtok.hpp, shared with bgin.hip);
//   rl_records              one thread per record: parse, the local checks (a contig starts at 0, start == previous end, end > start, value >= 0:
//                           they need the previous record's name and end only), run length and clamped value, contig starts, clamp count;
//   rl_scan_*               exclusive 64-bit scan of the run lengths (one feed of a few thousand bytes can describe more than 2^32 positions);
//   rl_tiles / rl_fill      the hot kernel: OUTPUT-tiled expansion into the flat uint16 array.  A block owns RL_TILE consecutive positions; the run
//                           that holds the first position of every tile is found by binary search in the scanned offsets (rl_tiles, one thread
//                           per tile); the block stages the starts and values of its runs in LDS; in each of two passes every lane owns 8
//                           consecutive positions, finds its run in LDS, walks on from there and writes one aligned 16-byte store.  One run
//                           of 242 M positions and 4096 runs of one position cost a tile the same; no atomics.
// Finish compares the contigs of the two files (count, names, lengths) and lays both flat arrays out with bg_layout (bgtok.hpp).
#include "bgtok.hpp"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_LANE = 8;                          // positions per lane and store: 16 bytes
constexpr int RL_PASSES = 2;                        // stores per lane
constexpr int RL_TILE = RL_THREADS * RL_LANE * RL_PASSES;   // positions a workgroup of rl_fill owns
static_assert(RL_TILE == CORNETTO_BGRUN_TILE, "the header publishes the tile size");

enum { RL_OK = 0, RL_COLUMNS = 1 /* + file */, RL_FIRST = 6, RL_GAP = 7, RL_EMPTY = 8, RL_NEGATIVE = 9, RL_PAIR = 10 };

struct RlArgs {
    const uint8_t *text;
    int64_t n;
    const uint32_t *tok;
    int64_t nrec;             // records in the buffer
    int32_t skip;             // leading records that are context only (already consumed): 0 or 1
    int32_t file_start;       // record 0 of the buffer is the first record of the file
    int32_t file;
    int64_t base;             // index in the file of record `skip`
    unsigned long long *len;  // [nrec - skip] run lengths (0 where a check failed: the feed is refused then)
    uint16_t *val;            // [nrec - skip]
    unsigned long long *err;  // min over records of (index in the file << 4 | kind), ~0 when clean
    uint32_t *n_break;
    uint4 *breaks;            // {record - skip, name offset, name length, -}
    uint32_t break_cap;
    unsigned long long *n_clamp;
};

// the checks of record r in their order -> kind (RL_OK: a run), the two numbers of the message
__device__ __forceinline__ int rl_check(const RlArgs &A, int64_t r, BgRec &x, bool &first, int &d0, int &d1)
{
    x = parse_rec(A.text, A.n, A.tok, r);
    d0 = d1 = 0;
    first = false;
    if (x.nfields != 4) { d0 = x.nfields; return RL_COLUMNS + A.file; }
    int32_t prev_end = 0;
    if (r == 0) {
        first = A.file_start != 0;   // (r == 0 without file_start is the context record: never checked)
    } else {
        uint32_t pl;
        const uint32_t po = name_of(A.text, A.n, A.tok, r - 1, &pl);
        first = !same_name(A.text, x.name_off, x.name_len, A.text, po, pl);
        if (!first) (void)parse_int(A.text, A.n, A.tok[4 * (r - 1) + 2], &prev_end);   // (a previous record that does not convert has the smaller index: it decides)
    }
    if (first && x.st != 0) { d0 = x.st; return RL_FIRST; }
    if (!first && x.st != prev_end) { d0 = prev_end; d1 = x.st; return RL_GAP; }
    if (x.end <= x.st) { d0 = x.st; d1 = x.end; return RL_EMPTY; }
    if (x.depth < 0) { d0 = x.depth; return RL_NEGATIVE; }
    return RL_OK;
}

__global__ __launch_bounds__(256) void rl_records(RlArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.nrec || r < A.skip) return;
    const int64_t j = r - A.skip;
    BgRec x;
    bool first;
    int d0, d1;
    const int kind = rl_check(A, r, x, first, d0, d1);
    if (kind != RL_OK) {
        atomicMin(A.err, ((unsigned long long)(A.base + j) << 4) | (unsigned)kind);
        A.len[j] = 0;
        A.val[j] = 0;
        return;
    }
    const unsigned long long len = (unsigned long long)((int64_t)x.end - (int64_t)x.st);
    A.len[j] = len;
    A.val[j] = (uint16_t)(x.depth > 65535 ? 65535 : x.depth);
    if (x.depth > 65535) atomicAdd(A.n_clamp, len);           // every position of the run counts, as in the per-base file
    if (first) {
        const uint32_t k = atomicAdd(A.n_break, 1u);
        if (k < A.break_cap) A.breaks[k] = make_uint4((uint32_t)j, x.name_off, x.name_len, 0u);
    }
}

// the numbers of the record that decided (one thread: the atomicMin above orders the keys, not the detail words)
__global__ void rl_detail(RlArgs A, int64_t r, int32_t *out)
{
    BgRec x;
    bool first;
    int d0, d1;
    (void)rl_check(A, r, x, first, d0, d1);
    out[0] = d0;
    out[1] = d1;
}

// ---- exclusive scan of 64-bit run lengths: tile-local scan, scan of the tile totals by one workgroup, offset add --------------------------
// (three launches: a 64-bit value does not fit the packed state of scan.hpp's look-back; the pieces inside a tile are the same)
constexpr int RS_ITEMS = 8;                         // run lengths per thread of the scan
constexpr int RS_TILE = RL_THREADS * RS_ITEMS;
static_assert(RL_THREADS == cnscan::SC_THREADS, "cnscan::tile_excl scans a workgroup of SC_THREADS");

__global__ __launch_bounds__(RL_THREADS) void rl_scan_tile(unsigned long long *io, int64_t n, unsigned long long *partial)
{
    const int64_t base = (int64_t)blockIdx.x * RS_TILE + (int64_t)threadIdx.x * RS_ITEMS;
    unsigned long long v[RS_ITEMS], total;
    const unsigned long long pre = cnscan::tile_excl(io, base, n, 1, v, total);
    cnscan::tile_write(io, base, n, pre, v);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void rl_scan_totals(unsigned long long *partial, int64_t np, unsigned long long *total)
{
    const int t = threadIdx.x;
    const int64_t per = (np + 1023) / 1024;
    const int64_t lo = (int64_t)t * per, hi = lo + per < np ? lo + per : np;
    unsigned long long s = 0, all;
    for (int64_t i = lo; i < hi; ++i) s += partial[i];
    unsigned long long run = cnscan::block_excl<unsigned long long, 1024>(s, all);
    for (int64_t i = lo; i < hi; ++i) {
        const unsigned long long x = partial[i];
        partial[i] = run;
        run += x;
    }
    if (t == 0) *total = all;
}

__global__ __launch_bounds__(RL_THREADS) void rl_scan_add(unsigned long long *io, int64_t n, const unsigned long long *partial)
{
    const unsigned long long add = partial[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
    for (int k = threadIdx.x; k < RS_TILE; k += RL_THREADS)
        if (base + k < n) io[base + k] += add;
}

// io[0 .. n) -> its exclusive prefix in place, *d_total = the sum; partial: room for ceil(n / RS_TILE) words
static int rl_scan(cornetto_accel_t *h, unsigned long long *io, int64_t n, unsigned long long *partial, unsigned long long *d_total)
{
    const int64_t np = (n + RS_TILE - 1) / RS_TILE;
    CN_LAUNCH(h, "rl_scan", rl_scan_tile<<<dim3((unsigned)np), dim3(RL_THREADS), 0, h->stream>>>(io, n, partial));
    CN_LAUNCH(h, "rl_scan", rl_scan_totals<<<dim3(1), dim3(1024), 0, h->stream>>>(partial, np, d_total));
    CN_LAUNCH(h, "rl_scan", rl_scan_add<<<dim3((unsigned)np), dim3(RL_THREADS), 0, h->stream>>>(io, n, partial));
    return CORNETTO_OK;
}

// contig starts: record -> first position of the record in the span
__global__ void rl_break_pos(const uint4 *breaks, uint32_t n, const unsigned long long *off, unsigned long long *pos)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) pos[k] = off[breaks[k].x];
}

// ---- the expansion ------------------------------------------------------------------------------------------------------------------
struct RlFill {
    const unsigned long long *off;   // [nrun] first position of every run in the span, strictly increasing (every run has a position)
    const uint16_t *val;             // [nrun]
    int64_t nrun;
    int64_t base;                    // position of the flat array where the span starts (wherever the last feed ended)
    int64_t total;                   // positions of the span
    uint16_t *dst;                   // the flat array
    uint32_t *first;                 // [tiles + 1] the run that holds the first position of every tile (rl_tiles)
    int64_t ntiles;
};

// Tiles are cut in the coordinates of the ARRAY, from `base` rounded down to 8 elements: a lane's 8 positions are one aligned 16-byte piece.
// The head of the first tile (in front of `base`) and the tail of the last one are not the span's: lanes that straddle them store by element.
__device__ __forceinline__ int64_t rl_tile_rel(const RlFill &A, int64_t tile) { return tile * RL_TILE - (A.base & (int64_t)(RL_LANE - 1)); }

// One thread per tile edge: the run that holds the first position of the tile, by binary search in the scanned offsets.  A kernel of its own:
// ~log2(runs) dependent loads in front of every tile's stores held rl_fill at a sixth of the fill rate; here a million searches hide each other.
__global__ __launch_bounds__(256) void rl_tiles(RlFill A)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > A.ntiles) return;
    const int64_t rel = rl_tile_rel(A, b);
    const int64_t p = rel < 0 ? 0 : rel;          // (beyond the span for b == ntiles: the last run)
    int64_t lo = 0, hi = A.nrun;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)A.off[mid] <= p) lo = mid; else hi = mid;
    }
    A.first[b] = (uint32_t)lo;
}

__global__ __launch_bounds__(RL_THREADS) void rl_fill(RlFill A)
{
    // the runs that overlap the tile — at most one per position — and the one that holds the next tile's first position (it may start there)
    __shared__ uint16_t s_start[RL_TILE + 2];     // first tile element of every staged run
    __shared__ uint16_t s_val[RL_TILE + 2];
    const int t = threadIdx.x;
    const int64_t rel = rl_tile_rel(A, blockIdx.x);                           // position in the span of tile element 0 (tile 0: -7 .. 0)
    uint16_t *const tile = A.dst + (A.base & ~(int64_t)(RL_LANE - 1)) + (int64_t)blockIdx.x * RL_TILE;
    const int x0 = rel < 0 ? (int)-rel : 0;                                   // the tile elements [x0, x1) belong to the span
    const int64_t left = A.total - rel;
    const int x1 = left < RL_TILE ? (int)left : RL_TILE;
    const int64_t r0 = A.first[blockIdx.x];
    const int cnt = (int)(A.first[blockIdx.x + 1] - r0) + 1;                  // <= RL_TILE + 1
    for (int i = t; i < cnt; i += RL_THREADS) {
        const int64_t s = (int64_t)A.off[r0 + i] - rel;                       // (<= RL_TILE: the last staged run holds element RL_TILE)
        s_start[i] = (uint16_t)(s < x0 ? x0 : s);
        s_val[i] = A.val[r0 + i];
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < RL_PASSES; ++pass) {      // a pass: the 256 lanes write 4 KB side by side
        const int xa = pass * (RL_THREADS * RL_LANE) + t * RL_LANE;
        const int xs = xa > x0 ? xa : x0, xe = xa + RL_LANE < x1 ? xa + RL_LANE : x1;
        if (xs >= xe) continue;
        int lo = 0, hi = cnt;                    // the run of the lane's first position: the last one that starts at or in front of it
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((int)s_start[mid] <= xs) lo = mid; else hi = mid;
        }
        int i = lo;
        uint32_t w[RL_LANE / 2] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < RL_LANE; ++k) {
            const int x = xa + k;
            uint32_t v = 0;
            if (x >= xs && x < xe) {
                while (i + 1 < cnt && (int)s_start[i + 1] <= x) ++i;
                v = s_val[i];
            }
            w[k >> 1] |= v << (16 * (k & 1));
        }
        uint16_t *d = tile + xa;
        if (xe - xs == RL_LANE) {
            *reinterpret_cast<uint4 *>(d) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < RL_LANE; ++k)
                if (xa + k >= xs && xa + k < xe) d[k] = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
        }
    }
}

}  // namespace

struct cornetto_bgrun {
    struct Brk { int64_t pos; std::string name; };
    struct File {
        std::string pend;          // the context record (the last consumed one) + bytes not yet consumed
        BgCarry dc;                // ... on the device instead, from the file's first compressed source on (cornetto_bgrun_feed_src)
        int32_t ctx = 0;           // context records at the head of pend: 0 or 1
        int64_t n_rec = 0, n_pos = 0;
        uint16_t *d = nullptr;     // the flat array
        int64_t cap = 0;
        std::vector<Brk> breaks;
        bool eof = false;
    } f[2];
    unsigned long long n_clamp = 0;
    cornetto_bgrunerr_t err{0, 0, 0, 0, 0};
};

namespace {

inline bool host_ws(unsigned char c) { return (unsigned)(c - 9) < 5u || c == 32; }

// parse_int's rule on the host (the tokens behind the last whole record of a file)
bool host_token_is_int(const std::string &s, size_t p)
{
    if (p < s.size() && (s[p] == '-' || s[p] == '+')) ++p;
    if (p >= s.size() || s[p] < '0' || s[p] > '9') return false;
    while (p < s.size() && s[p] >= '0' && s[p] <= '9') ++p;
    return p >= s.size() || host_ws((unsigned char)s[p]);
}

int rl_format_error(cornetto_accel_t *h, cornetto_bgrun_t *b, int kind, int file, int64_t record, int32_t a, int32_t c)
{
    b->err = cornetto_bgrunerr_t{kind, file, record, a, c};
    cn_timing_end(h);
    return CORNETTO_E_FORMAT;
}

}  // namespace

extern "C" {

int32_t cornetto_bgrun_tile(void) { return RL_TILE; }

int cornetto_bgrun_open(cornetto_accel_t *h, cornetto_bgrun_t **out)
{
    if (!h || !out) return cn_fail(h, CORNETTO_E_ARG, "bgrun_open: bad argument");
    *out = new (std::nothrow) cornetto_bgrun;
    return *out ? CORNETTO_OK : cn_fail(h, CORNETTO_E_NOMEM, "bgrun_open: host allocation failed");
}

void cornetto_bgrun_close(cornetto_accel_t *h, cornetto_bgrun_t *b)
{
    if (!b) return;
    if (h) (void)hipSetDevice(h->device);
    for (auto &f : b->f) {
        if (f.d) (void)hipFree(f.d);
        f.dc.release();
    }
    delete b;
}

const cornetto_bgrunerr_t *cornetto_bgrun_error(const cornetto_bgrun_t *b) { return b ? &b->err : nullptr; }

}  // extern "C"

// The feed over a source (cornetto_bgsrc_t), plain host bytes or BGZF blocks on the device: what cornetto_bgrun_feed() and
// cornetto_bgrun_feed_src() run.  A file that has had a compressed source keeps its carry on the device (BgCarry) from then on.
static int bgrun_feed_core(cornetto_accel_t *h, cornetto_bgrun_t *b, int file, const cornetto_bgsrc_t *S, int final)
{
    if (b->err.kind) return CORNETTO_E_FORMAT;
    cornetto_bgrun::File &F = b->f[file];
    int64_t n_new = 0;
    if (!bgsrc_size(S, &n_new)) return cn_fail(h, CORNETTO_E_ARG, "bgrun_feed: bad source");
    const bool comp = bgsrc_compressed(S);
    const char *text = comp || !S ? nullptr : S->text;
    if (F.eof) return n_new == 0 && !comp ? CORNETTO_OK : cn_fail(h, CORNETTO_E_ARG, "bgrun_feed: file %d has had its final feed", file);
    // (the work space slots are the per-base reader's: the contents of a slot do not outlive a call)
    const int64_t n_pend = F.dc.on ? F.dc.n : (int64_t)F.pend.size();
    int64_t n = n_pend + n_new;
    if (n > 0xF0000000ll) return cn_fail(h, CORNETTO_E_ARG, "bgrun_feed: more than 3.75 GiB pending; feed smaller pieces");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    if (comp && !F.dc.on) {   // the file's first compressed source: what it carries moves to the device and stays there
        CN_TRY(bg_carry_from_host(h, F.dc, F.pend));
        F.pend.clear();
    }
    uint8_t *d_text = (uint8_t *)cn_ws(h, WS_BG_TEXT_A, (size_t)n + 64);
    if (!d_text) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: workspace allocation failed");
    if (F.dc.on) {
        if (n_pend) CN_HIP(h, hipMemcpyAsync(d_text, F.dc.d, (size_t)n_pend, hipMemcpyDeviceToDevice, h->stream));
    } else if (n_pend) CN_HIP(h, hipMemcpyAsync(d_text, F.pend.data(), (size_t)n_pend, hipMemcpyHostToDevice, h->stream));
    int64_t bad = -1;   // the first block of this feed that is not what its footer says
    if (comp) {
        // its blocks inflate behind the carry, in the text workspace itself; the text ends in front of a bad block, and the file is not at its
        // end there: the last token in front of the block counts as cut
        int64_t good = 0;
        CN_TRY(bgsrc_inflate(h, S, d_text, n_pend, &bad, &good));
        if (bad >= 0) {
            n = n_pend + good;
            final = 0;
        }
    } else if (n_new) CN_HIP(h, hipMemcpyAsync(d_text + n_pend, text, (size_t)n_new, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_tok = nullptr;
    int64_t all_tok = 0;
    CN_TRY(tokenize(h, d_text, n, WS_BG_TOK_A, WS_BG_CNT_A, &d_tok, &all_tok));
    int64_t ntok = all_tok;
    {   // a token cut by the end of the buffer is not complete yet (unless this is the end of the file)
        int lb = ' ';
        if (n > 0) {
            if (F.dc.on) CN_TRY(bg_byte_at(h, d_text, n - 1, &lb));      // (the device text: inflated bytes have no copy on the host)
            else lb = n_new ? (unsigned char)text[n_new - 1] : (unsigned char)F.pend.back();
        }
        if (!final && !host_ws((unsigned char)lb) && ntok > 0) --ntok;
    }
    const int64_t nrec = ntok / 4, fresh = nrec - F.ctx;
    auto byte_at = [&](int64_t off, int64_t len) -> std::string {   // bytes [off, off + len) of (pend | new data)
        std::string s;
        if (len <= 0) return s;
        if (F.dc.on) {   // from the device text (a few bytes behind the last record of a file; the names of a feed come packed: bg_fetch_names)
            s.resize((size_t)len);
            if (hipMemcpyAsync(&s[0], d_text + off, (size_t)len, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
                s.assign((size_t)len, ' ');
            return s;
        }
        s.reserve((size_t)len);
        if (off < n_pend) s.append(F.pend, (size_t)off, (size_t)std::min<int64_t>(len, n_pend - off));
        if (off + len > n_pend) {
            const int64_t o2 = std::max<int64_t>(off, n_pend) - n_pend;
            s.append(text + o2, (size_t)(off + len - n_pend - o2));
        }
        return s;
    };
    if (fresh > 0) {
        unsigned long long *d_small = (unsigned long long *)cn_ws(h, WS_BG_SMALL, 256);
        unsigned long long *p_small = (unsigned long long *)cn_pin(h, PIN_SMALL, 256);
        const int64_t np = (fresh + RS_TILE - 1) / RS_TILE;
        // run offsets [fresh], tile totals [np], values [fresh]
        unsigned long long *d_off = (unsigned long long *)cn_ws(h, WS_BG_TEXT_B, ((size_t)fresh + (size_t)np + 2) * 8 + (size_t)fresh * 2 + 16);
        if (!d_small || !p_small || !d_off) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: workspace allocation failed");
        unsigned long long *d_part = d_off + fresh;
        uint16_t *d_val = reinterpret_cast<uint16_t *>(d_part + np + 1);
        uint32_t break_cap = 1u << 16, nb = 0;
        uint4 *d_brk = nullptr;
        RlArgs A{};
        for (int attempt = 0; attempt < 2; ++attempt) {
            d_brk = (uint4 *)cn_ws(h, WS_BG_BRK, (size_t)break_cap * (sizeof(uint4) + 8));
            if (!d_brk) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: workspace allocation failed");
            CN_HIP(h, hipMemsetAsync(d_small, 0, 256, h->stream));
            CN_HIP(h, hipMemsetAsync(d_small, 0xFF, 8, h->stream));
            A = RlArgs{d_text, n, d_tok, nrec, F.ctx, F.ctx == 0 && F.n_rec == 0 ? 1 : 0, file, F.n_rec, d_off, d_val,
                       d_small, reinterpret_cast<uint32_t *>(d_small + 1), d_brk, break_cap, d_small + 2};
            CN_LAUNCH(h, "rl_records", rl_records<<<dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, h->stream>>>(A));
            CN_HIP(h, hipMemcpyAsync(p_small, d_small, 24, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            nb = (uint32_t)(p_small[1] & 0xFFFFFFFFull);
            if (nb <= break_cap) break;
            if (attempt == 1) return cn_fail(h, CORNETTO_E_HIP, "bgrun_feed: contig-start list overflow");
            break_cap = nb;   // more contig starts than room: exact rerun (the kernel is idempotent)
        }
        if (p_small[0] != ~0ull) {   // the record with the smallest index that fails a check decides
            const int64_t rec = (int64_t)(p_small[0] >> 4);
            int32_t *d_det = reinterpret_cast<int32_t *>(d_small + 4);
            rl_detail<<<dim3(1), dim3(1), 0, h->stream>>>(A, rec - F.n_rec + F.ctx, d_det);
            CN_HIP(h, hipGetLastError());
            CN_HIP(h, hipMemcpyAsync(p_small + 4, d_det, 8, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            const int32_t *det = reinterpret_cast<const int32_t *>(p_small + 4);
            return rl_format_error(h, b, (int)(p_small[0] & 15), file, rec, det[0], det[1]);
        }
        const unsigned long long clamped = p_small[2];
        CN_TRY(rl_scan(h, d_off, fresh, d_part, d_small + 3));
        unsigned long long *d_bpos = reinterpret_cast<unsigned long long *>(d_brk + break_cap);
        if (nb) {
            rl_break_pos<<<dim3((nb + 255) / 256), dim3(256), 0, h->stream>>>(d_brk, nb, d_off, d_bpos);
            CN_HIP(h, hipGetLastError());
        }
        CN_HIP(h, hipMemcpyAsync(p_small + 3, d_small + 3, 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        const int64_t total = (int64_t)p_small[3];
        if (total < 0 || total > (int64_t)1 << 46) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: one piece of text describes %lld positions", (long long)total);
        if (F.n_pos + total > F.cap) {   // grow the flat array (amortised doubling)
            const int64_t ncap = std::max<int64_t>(F.cap * 2, F.n_pos + total + (1 << 20));
            uint16_t *nd = nullptr;
            if (hipMalloc((void **)&nd, (size_t)ncap * 2) != hipSuccess)
                return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: cannot grow the depth array of file %d to %lld positions", file, (long long)ncap);
            if (F.n_pos) {
                CN_HIP(h, hipMemcpyAsync(nd, F.d, (size_t)F.n_pos * 2, hipMemcpyDeviceToDevice, h->stream));
                CN_HIP(h, hipStreamSynchronize(h->stream));
            }
            if (F.d) (void)hipFree(F.d);
            F.d = nd;
            F.cap = ncap;
        }
        {
            const int64_t head = F.n_pos & (RL_LANE - 1);
            const int64_t nt = (head + total + RL_TILE - 1) / RL_TILE;
            uint32_t *d_first = (uint32_t *)cn_ws(h, WS_BG_TOK_B, ((size_t)nt + 1) * 4);
            if (!d_first) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_feed: workspace allocation failed");
            RlFill Fa{d_off, d_val, fresh, F.n_pos, total, F.d, d_first, nt};
            CN_LAUNCH(h, "rl_tiles", rl_tiles<<<dim3((unsigned)((nt + 256) / 256)), dim3(256), 0, h->stream>>>(Fa));
            CN_LAUNCH(h, "rl_fill", rl_fill<<<dim3((unsigned)nt), dim3(RL_THREADS), 0, h->stream>>>(Fa));
        }
        std::vector<uint4> brk(nb);
        std::vector<unsigned long long> bpos(nb);
        if (nb) {
            CN_HIP(h, hipMemcpyAsync(brk.data(), d_brk, (size_t)nb * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipMemcpyAsync(bpos.data(), d_bpos, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
        }
        CN_HIP(h, hipStreamSynchronize(h->stream));
        const size_t at = F.breaks.size();
        std::vector<std::string> dev_names;
        if (F.dc.on) CN_TRY(bg_fetch_names(h, d_text, d_brk, brk, 1, &dev_names));
        for (uint32_t k = 0; k < nb; ++k) F.breaks.push_back(cornetto_bgrun::Brk{F.n_pos + (int64_t)bpos[k], F.dc.on ? dev_names[k] : byte_at(brk[k].y, brk[k].z)});
        std::sort(F.breaks.begin() + (std::ptrdiff_t)at, F.breaks.end(), [](const cornetto_bgrun::Brk &x, const cornetto_bgrun::Brk &y) { return x.pos < y.pos; });
        b->n_clamp += clamped;
        F.n_pos += total;
        F.n_rec += fresh;
    }
    if (bad >= 0) {   // every record in front of the block has passed its checks: the block itself is what is wrong
        const int64_t at = S->blocks[bad].src;
        return rl_format_error(h, b, BG_BLOCK, file, F.dc.blocks + bad, (int32_t)(uint32_t)(at & 0xFFFFFFFFll), (int32_t)(at >> 32));
    }
    if (comp) F.dc.blocks += S->n_blocks;
    // the tokens behind the last whole record, and where the carry starts
    const int64_t t_cut = 4 * nrec, n_left = all_tok - t_cut;
    uint32_t v[4] = {0, 0, 0, 0};   // [0..2]: the first tokens that are left, [3]: the last consumed record
    if (n_left > 0) CN_HIP(h, hipMemcpy(v, d_tok + t_cut, (size_t)std::min<int64_t>(n_left, 3) * 4, hipMemcpyDeviceToHost));
    if (nrec > 0) CN_HIP(h, hipMemcpy(&v[3], d_tok + 4 * (nrec - 1), 4, hipMemcpyDeviceToHost));
    if (final) {
        if (n_left >= 1) {   // 1..3 tokens: a record with fewer than four converted fields
            const std::string rest = byte_at(v[0], n - v[0]);   // (v[0]: the first of those tokens)
            int conv = 1;
            if (n_left >= 2 && host_token_is_int(rest, v[1] - v[0])) {
                conv = 2;
                if (n_left >= 3 && host_token_is_int(rest, v[2] - v[0])) conv = 3;
            }
            return rl_format_error(h, b, RL_COLUMNS + file, file, F.n_rec, conv, 0);
        }
        F.eof = true;
        F.pend.clear();
        F.dc.n = 0;
        F.ctx = 0;
    } else {
        const int64_t cut = n_left > 0 ? (int64_t)v[0] : n;
        const int64_t from = nrec > 0 ? (int64_t)v[3] : cut;
        if (F.dc.on) {
            CN_TRY(bg_carry_store(h, F.dc, d_text + from, n - from));
            CN_HIP(h, hipStreamSynchronize(h->stream));   // (the carry has left the text workspace)
        } else {
            std::string np = byte_at(from, n - from);
            F.pend.swap(np);
        }
        F.ctx = nrec > 0 ? 1 : 0;
    }
    cn_timing_end(h);
    return CORNETTO_OK;
}

extern "C" {

int cornetto_bgrun_feed(cornetto_accel_t *h, cornetto_bgrun_t *b, int file, const char *text, int64_t n_new, int final)
{
    if (!h || !b || file < 0 || file > 1 || n_new < 0 || (n_new > 0 && !text)) return cn_fail(h, CORNETTO_E_ARG, "bgrun_feed: bad argument");
    const cornetto_bgsrc_t s{text, n_new, nullptr, nullptr, 0};
    return bgrun_feed_core(h, b, file, &s, final);
}

int cornetto_bgrun_feed_src(cornetto_accel_t *h, cornetto_bgrun_t *b, int file, const cornetto_bgsrc_t *src, int final)
{
    if (!h || !b || file < 0 || file > 1) return cn_fail(h, CORNETTO_E_ARG, "bgrun_feed_src: bad argument");
    return bgrun_feed_core(h, b, file, src, final);
}

int cornetto_bgrun_finish(cornetto_accel_t *h, cornetto_bgrun_t *b, cornetto_cov_t **cov, int32_t *n_ctg, char ***names, int64_t *n_clamped)
{
    if (!h || !b || !cov || !n_ctg || !names) return cn_fail(h, CORNETTO_E_ARG, "bgrun_finish: bad argument");
    if (b->err.kind) return CORNETTO_E_FORMAT;
    if (!b->f[0].eof || !b->f[1].eof) return cn_fail(h, CORNETTO_E_ARG, "bgrun_finish: both files need a feed with final = 1");
    CN_HIP(h, hipSetDevice(h->device));
    *cov = nullptr;
    *n_ctg = 0;
    *names = nullptr;
    if (n_clamped) *n_clamped = (int64_t)b->n_clamp;
    // the two files against each other: contig k of both has the same name and the same length
    const size_t n0 = b->f[0].breaks.size(), n1 = b->f[1].breaks.size();
    auto len_of = [&](int f, size_t k) -> int64_t {
        const auto &br = b->f[f].breaks;
        return k >= br.size() ? 0 : (k + 1 < br.size() ? br[k + 1].pos : b->f[f].n_pos) - br[k].pos;
    };
    if (std::max(n0, n1) > (size_t)INT32_MAX) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "bgrun_finish: more than 2^31-1 contigs");
    for (size_t k = 0; k < std::max(n0, n1); ++k) {
        const int64_t l0 = len_of(0, k), l1 = len_of(1, k);
        if (l0 > INT32_MAX || l1 > INT32_MAX) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "bgrun_finish: contig %zu has more than 2^31-1 positions", k);
        if (k >= n0 || k >= n1 || l0 != l1 || b->f[0].breaks[k].name != b->f[1].breaks[k].name) {
            b->err = cornetto_bgrunerr_t{RL_PAIR, 0, (int64_t)k, (int32_t)l0, (int32_t)l1};
            return CORNETTO_E_FORMAT;
        }
    }
    const int32_t nc = (int32_t)n0;
    cornetto_cov_t *c = new (std::nothrow) cornetto_cov;
    if (!c) return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_finish: host allocation failed");
    c->n = nc;
    std::vector<int64_t> src_off(nc), lens(nc);
    for (int32_t i = 0; i < nc; ++i) {
        src_off[i] = b->f[0].breaks[i].pos;
        lens[i] = len_of(0, (size_t)i);
    }
    const int rc = bg_cov_layout(h, "bgrun_finish", c, b->f[0].d, b->f[1].d, src_off, lens);
    if (rc != CORNETTO_OK) return rc;
    for (auto &f : b->f) {   // the flat arrays are no longer needed
        if (f.d) (void)hipFree(f.d);
        f.d = nullptr;
        f.cap = 0;
    }
    char **nm = (char **)malloc((size_t)(nc > 0 ? nc : 1) * sizeof(char *));
    if (!nm) { cornetto_cov_free(h, c); return cn_fail(h, CORNETTO_E_NOMEM, "bgrun_finish: host allocation failed"); }
    for (int32_t i = 0; i < nc; ++i) {
        const std::string &s = b->f[0].breaks[i].name;
        nm[i] = (char *)malloc(s.size() + 1);
        if (nm[i]) memcpy(nm[i], s.c_str(), s.size() + 1);
    }
    *cov = c;
    *n_ctg = nc;
    *names = nm;
    return CORNETTO_OK;
}

#ifdef CN_DEV
// development build only (selftest.hip, tests/test_gpu_scan.py): the 64-bit scan of the feed path on its own — io[0 .. n) (host) becomes
// its exclusive prefix, *total the sum
int cn_selftest_scan_u64(cornetto_accel_t *h, unsigned long long *io, int64_t n, unsigned long long *total)
{
    if (!h || !io || !total || n <= 0 || n > ((int64_t)1 << 28)) return cn_fail(h, CORNETTO_E_ARG, "selftest_scan_u64: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t np = (n + RS_TILE - 1) / RS_TILE;
    DevBuf d;
    if (d.alloc(((size_t)n + (size_t)np + 1) * 8) != hipSuccess) return cn_fail(h, CORNETTO_E_NOMEM, "selftest: device allocation failed");
    unsigned long long *d_io = d.as<unsigned long long>(), *d_part = d_io + n;
    CN_HIP(h, hipMemcpyAsync(d_io, io, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    CN_TRY(rl_scan(h, d_io, n, d_part, d_part + np));
    CN_HIP(h, hipMemcpyAsync(io, d_io, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipMemcpyAsync(total, d_part + np, 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    return CORNETTO_OK;
}
#endif

}  // extern "C"
