// emit.hip — `cornetto fixasm`'s output text on the device (include/cornetto_accel.h: cornetto_emit_*).
//
// The text of a plan is, for every record r of an ordered list, heads[r] + the bases of contig r.ctg of a resident assembly, forward or
// reverse-complemented as src/fixasm.c:208-224 does it (reversed; only the upper-case A<->T, C<->G complemented), + '\n'.  That is what
// fix_the_assembly() prints with ">%s_%d\n%s\n" (src/fixasm.c:384).  Any byte window [at, at + n) of it is written into a device slab and
// copied to the caller's pinned memory on one of four copy queues, so the kernel of the next window runs beside the copy of this one.
//
// Work decomposition: a block writes a tile of EMIT_TILE consecutive output bytes, a thread 16 bytes at a time with one vector store (the
// window starts at a slab offset of 0, so every store is 16-byte aligned).  The records of a tile come from a binary search of the output-offset
// table: once per tile for its first and last byte (uniform: scalar loads), then per 16-byte chunk inside that short range.  A chunk that lies
// inside the bases of one record reads them with two aligned 16-byte loads merged by alignbyte (its source offset is arbitrary: the output offsets
// are), reversed with perm and complemented with a SWAR select; any other chunk (a header, a newline, a record border, the window's end) is
// written byte by byte.
//
// Reads stay inside what cornetto_asm_wrap guarantees: a contig starts at a multiple of 64 of the buffer, and 128 bytes past the last contig are
// readable.  The forward loads of a chunk end at most 31 bytes past its first source byte, whose chunk ends inside the contig; the reverse
// loads begin at the aligned-down address of a byte that is inside the contig, never below its (64-aligned) start.
#include "common.hpp"

namespace {

constexpr int EMIT_THREADS = 256;
constexpr int EMIT_PER_THREAD = 4;                                       // 16-byte chunks per thread
constexpr int64_t EMIT_TILE = (int64_t)EMIT_THREADS * 16 * EMIT_PER_THREAD;   // 16 KiB of output per block

struct EmitRec {
    int64_t src;    // offset of the contig's first base in the assembly's buffer
    int64_t head;   // offset of the record's header in the head bytes
    int32_t hl;     // header bytes
    int32_t len;    // bases
    int32_t rc;     // reverse-complemented
    int32_t pad;
};

struct EmitArgs {
    const uint8_t *bases;
    const int64_t *out;     // [n + 1]: first output byte of every record, then the total
    const EmitRec *recs;
    const uint8_t *heads;
    int64_t n;
    int64_t at, nbytes;
    uint8_t *dst;
};

// largest r in [lo, hi] with out[r] <= p (out is strictly increasing: a record is at least its newline)
__device__ inline int64_t emit_find(const int64_t *out, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (out[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// 0xFF in every byte of x that equals the byte of the broadcast pattern, else 0 (no carries between bytes: (t & 0x7F) + 0x7F <= 0xFE)
__device__ inline uint32_t emit_eq(uint32_t x, uint32_t pat)
{
    const uint32_t t = x ^ pat;
    const uint32_t y = ((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t;
    return ((~y & 0x80808080u) >> 7) * 0xFFu;
}

// A (0x41) <-> T (0x54) differ by 0x15, C (0x43) <-> G (0x47) by 0x04; every other byte is kept (src/fixasm.c:216-222)
__device__ inline uint32_t emit_comp4(uint32_t x)
{
    const uint32_t at = emit_eq(x, 0x41414141u) | emit_eq(x, 0x54545454u);
    const uint32_t cg = emit_eq(x, 0x43434343u) | emit_eq(x, 0x47474747u);
    return x ^ (at & 0x15151515u) ^ (cg & 0x04040404u);
}

__device__ inline uint8_t emit_comp1(uint8_t c)
{
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'C' ? 'G' : c;
}

// 16 bytes from an arbitrary address: the two aligned 16-byte vectors that hold them, merged
__device__ inline uint4 emit_load16(const uint8_t *p)
{
    const uintptr_t a = (uintptr_t)p;
    const uint4 *q = reinterpret_cast<const uint4 *>(a & ~(uintptr_t)15);
    const uint4 A = q[0], B = q[1];
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    const int ws = (int)(a >> 2) & 3, sb = (int)a & 3;
    uint32_t v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = ws == 0 ? w[k] : ws == 1 ? w[k + 1] : ws == 2 ? w[k + 2] : w[k + 3];
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(v[1], v[0], sb);
    o.y = __builtin_amdgcn_alignbyte(v[2], v[1], sb);
    o.z = __builtin_amdgcn_alignbyte(v[3], v[2], sb);
    o.w = __builtin_amdgcn_alignbyte(v[4], v[3], sb);
    return o;
}

__device__ inline uint32_t emit_bswap(uint32_t x) { return __builtin_amdgcn_perm(0u, x, 0x00010203u); }

__device__ inline uint8_t emit_byte(const EmitArgs &A, const EmitRec &r, int64_t k)   // byte k of record r's text
{
    if (k < r.hl) return A.heads[r.head + k];
    k -= r.hl;
    if (k >= r.len) return '\n';
    return r.rc ? emit_comp1(A.bases[r.src + r.len - 1 - k]) : A.bases[r.src + k];
}

__global__ __launch_bounds__(EMIT_THREADS) void emit_text(EmitArgs A)
{
    const int64_t tile = (int64_t)blockIdx.x * EMIT_TILE;
    const int64_t t_end = (A.nbytes - tile < EMIT_TILE ? A.nbytes - tile : EMIT_TILE);
    const int64_t r0 = emit_find(A.out, 0, A.n - 1, A.at + tile);
    const int64_t r1 = emit_find(A.out, r0, A.n - 1, A.at + tile + t_end - 1);
#pragma unroll
    for (int u = 0; u < EMIT_PER_THREAD; ++u) {
        const int64_t rel = tile + ((int64_t)u * EMIT_THREADS + threadIdx.x) * 16;
        if (rel >= tile + t_end) break;
        const int64_t p = A.at + rel;
        int64_t ri = emit_find(A.out, r0, r1, p);
        const EmitRec r = A.recs[ri];
        const int64_t b0 = p - A.out[ri] - r.hl;   // base index of the chunk's first byte
        if (b0 >= 0 && b0 + 16 <= r.len && rel + 16 <= A.nbytes) {
            uint4 v;
            if (!r.rc) {
                v = emit_load16(A.bases + r.src + b0);
            } else {
                const uint4 s = emit_load16(A.bases + r.src + (r.len - 16 - b0));
                v.x = emit_comp4(emit_bswap(s.w));
                v.y = emit_comp4(emit_bswap(s.z));
                v.z = emit_comp4(emit_bswap(s.y));
                v.w = emit_comp4(emit_bswap(s.x));
            }
            *reinterpret_cast<uint4 *>(A.dst + rel) = v;
            continue;
        }
        const int m = (int)(A.nbytes - rel < 16 ? A.nbytes - rel : 16);
        EmitRec cur = r;
        int64_t o = A.out[ri], o1 = A.out[ri + 1];
        for (int j = 0; j < m; ++j) {
            const int64_t q = p + j;
            while (q >= o1) {               // (q < total = out[n]: never past the last record)
                ++ri;
                cur = A.recs[ri];
                o = o1;
                o1 = A.out[ri + 1];
            }
            A.dst[rel + j] = emit_byte(A, cur, q - o);
        }
    }
}

}  // namespace

struct cornetto_emit {
    const uint8_t *bases = nullptr;    // the assembly's buffer (borrowed)
    int64_t n = 0, total = 0;
    int64_t *d_out = nullptr;
    EmitRec *d_recs = nullptr;
    uint8_t *d_heads = nullptr;
    uint8_t *slab[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t slab_cap[4] = {0, 0, 0, 0};
    hipStream_t q[4] = {nullptr, nullptr, nullptr, nullptr};   // kernel + copy of slot s, in order
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // the last copy of slot s
};

extern "C" void cornetto_emit_free(cornetto_accel_t *h, cornetto_emit_t *e)
{
    if (!e) return;
    if (h) (void)hipSetDevice(h->device);
    for (int i = 0; i < 4; ++i)
        if (e->q[i]) { (void)hipStreamSynchronize(e->q[i]); (void)hipStreamDestroy(e->q[i]); }
    for (int i = 0; i < 4; ++i) {
        if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
        if (e->slab[i]) (void)hipFree(e->slab[i]);
    }
    if (e->d_out) (void)hipFree(e->d_out);
    if (e->d_recs) (void)hipFree(e->d_recs);
    if (e->d_heads) (void)hipFree(e->d_heads);
    delete e;
}

extern "C" int cornetto_emit_open(cornetto_accel_t *h, const cornetto_asm_t *a, const cornetto_emit_rec_t *recs, int64_t n, const char *heads, int64_t n_heads,
                                  cornetto_emit_t **out, int64_t *total_bytes)
{
    if (!h || !a || !out || !total_bytes || n < 0 || n_heads < 0 || (n > 0 && !recs) || (n_heads > 0 && !heads))
        return cn_fail(h, CORNETTO_E_ARG, "emit_open: bad argument");
    *out = nullptr;
    *total_bytes = 0;
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<EmitRec> tab((size_t)n);
    int64_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        const cornetto_emit_rec_t &r = recs[i];
        if (r.ctg < 0 || r.ctg >= a->n || r.head < 0 || r.head_len < 0 || r.head_len > INT32_MAX || r.head > n_heads - r.head_len)
            return cn_fail(h, CORNETTO_E_ARG, "emit_open: record %lld: contig %d of %d, head [%lld, +%lld) of %lld bytes", (long long)i, r.ctg, a->n,
                           (long long)r.head, (long long)r.head_len, (long long)n_heads);
        EmitRec &t = tab[(size_t)i];
        t.src = a->off[(size_t)r.ctg];
        t.head = r.head;
        t.hl = (int32_t)r.head_len;
        t.len = a->len[(size_t)r.ctg];
        t.rc = r.rc != 0;
        t.pad = 0;
        off[(size_t)i] = pos;
        pos += r.head_len + t.len + 1;
    }
    off[(size_t)n] = pos;
    CN_HIP(h, hipSetDevice(h->device));
    cornetto_emit_t *e = new (std::nothrow) cornetto_emit;
    if (!e) return cn_fail(h, CORNETTO_E_NOMEM, "emit_open: host allocation failed");
    e->bases = a->d_bases;
    e->n = n;
    e->total = pos;
    bool ok = hipMalloc((void **)&e->d_out, ((size_t)n + 1) * sizeof(int64_t)) == hipSuccess &&
              hipMalloc((void **)&e->d_recs, ((size_t)n + 1) * sizeof(EmitRec)) == hipSuccess &&
              hipMalloc((void **)&e->d_heads, (size_t)n_heads + 16) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipStreamCreateWithFlags(&e->q[i], hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipEventCreateWithFlags(&e->ev[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipEventRecord(e->ev[i], e->q[i]) == hipSuccess;   // (a wait on a slot that has had no get returns at once)
    if (!ok) {
        cornetto_emit_free(h, e);
        return cn_fail(h, CORNETTO_E_NOMEM, "emit_open: device allocation for %lld records failed", (long long)n);
    }
    hipError_t err = hipMemcpy(e->d_out, off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    if (err == hipSuccess && n > 0) err = hipMemcpy(e->d_recs, tab.data(), (size_t)n * sizeof(EmitRec), hipMemcpyHostToDevice);
    if (err == hipSuccess && n_heads > 0) err = hipMemcpy(e->d_heads, heads, (size_t)n_heads, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipStreamSynchronize(h->stream);     // the assembly's bases are in place (filled on the handle's stream)
    if (err != hipSuccess) {
        cornetto_emit_free(h, e);
        return cn_fail(h, CORNETTO_E_HIP, "emit_open: copying the plan failed: %s", hipGetErrorString(err));
    }
    *out = e;
    *total_bytes = pos;
    return CORNETTO_OK;
}

extern "C" int cornetto_emit_get(cornetto_accel_t *h, cornetto_emit_t *e, char *dst_pinned, int64_t at, int64_t n, int slot)
{
    if (!h || !e || at < 0 || n < 0 || at > e->total - n || slot < 0 || slot > 3 || (n > 0 && !dst_pinned))
        return cn_fail(h, CORNETTO_E_ARG, "emit_get: bad argument");
    if (n == 0) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    hipStream_t q = e->q[slot];
    const int64_t need = cn_align_up(n, 16);
    if (e->slab_cap[slot] < need) {              // (the slot's last copy out of the old slab must be through first)
        CN_HIP(h, hipStreamSynchronize(q));
        if (e->slab[slot]) (void)hipFree(e->slab[slot]);
        e->slab[slot] = nullptr;
        e->slab_cap[slot] = 0;
        if (hipMalloc((void **)&e->slab[slot], (size_t)need) != hipSuccess) {
            e->slab[slot] = nullptr;
            return cn_fail(h, CORNETTO_E_NOMEM, "emit_get: device slab of %lld bytes", (long long)need);
        }
        e->slab_cap[slot] = need;
    }
    EmitArgs A{e->bases, e->d_out, e->d_recs, e->d_heads, e->n, at, n, e->slab[slot]};
    const int64_t blocks = (n + EMIT_TILE - 1) / EMIT_TILE;
    if (blocks > INT32_MAX) return cn_fail(h, CORNETTO_E_ARG, "emit_get: window of %lld bytes is too large", (long long)n);
    emit_text<<<dim3((unsigned)blocks), dim3(EMIT_THREADS), 0, q>>>(A);
    CN_HIP(h, hipGetLastError());
    CN_HIP(h, hipMemcpyAsync(dst_pinned, e->slab[slot], (size_t)n, hipMemcpyDeviceToHost, q));
    CN_HIP(h, hipEventRecord(e->ev[slot], q));
    return CORNETTO_OK;
}

extern "C" int cornetto_emit_wait(cornetto_accel_t *h, cornetto_emit_t *e, int slot)
{
    if (!h || !e || slot < 0 || slot > 3) return cn_fail(h, CORNETTO_E_ARG, "emit_wait: bad argument");
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipEventSynchronize(e->ev[slot]));
    return CORNETTO_OK;
}
