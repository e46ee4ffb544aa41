// bgtok.hpp — what the two bedgraph readers share (bgin.hip: the lock-step per-base pair; bgrun.hip: run-length files): the tokeniser
// (a record is FOUR WHITE-SPACE SEPARATED TOKENS, as fscanf("%s\t%d\t%d\t%d\n") reads them), the %d conversion of one token, the name
// helpers, and the way from the flat depth arrays of an ingest to the 64-element aligned layout of cornetto_cov_t.
#pragma once
#include <algorithm>
#include <string>

#include <vector>

#include "common.hpp"
#include "internal.hpp"
#include "marks.hpp"

namespace {   // internal linkage: every translation unit that includes this gets its own copy

__device__ __forceinline__ bool is_ws(uint32_t c) { return (c - 9u < 5u) | (c == 32u); }   // isspace() in the C locale

// bit i = byte i of the 16-byte piece at `pos` is white space; bytes at or beyond n count as white space
__device__ __forceinline__ uint32_t ws_mask16(const uint8_t *text, int64_t pos, int64_t n)
{
    uint32_t m = 0;
    if (pos + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) m |= (uint32_t)is_ws((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) << i;
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) m |= (uint32_t)(pos + i >= n || is_ws(text[pos + i])) << i;
    }
    return m;
}

__device__ __forceinline__ uint32_t tokstart_mask(const uint8_t *text, int64_t pos, int64_t n)
{
    if (pos >= n) return 0;
    const uint32_t ws = ws_mask16(text, pos, n);
    const uint32_t prev = pos == 0 ? 1u : (uint32_t)is_ws(text[pos - 1]);
    return ~ws & ((ws << 1) | prev) & 0xFFFFu;
}

// %d of one token: optional sign, digits up to the next white space; anything else fails the conversion
__device__ __forceinline__ bool parse_int(const uint8_t *text, int64_t n, uint32_t pos, int32_t *out)
{
    int64_t p = pos;
    bool neg = false;
    if (p < n && (text[p] == '-' || text[p] == '+')) neg = text[p++] == '-';
    if (p >= n || text[p] < '0' || text[p] > '9') return false;
    uint32_t v = 0;
    while (p < n && text[p] >= '0' && text[p] <= '9') v = v * 10u + (uint32_t)(text[p++] - '0');
    if (p < n && !is_ws(text[p])) return false;
    *out = (int32_t)(neg ? 0u - v : v);
    return true;
}

struct BgRec {
    uint32_t name_off, name_len;
    int32_t st, end, depth;
    int32_t nfields;      // converted fields, like the return value of the reference's fscanf
};

__device__ __forceinline__ BgRec parse_rec(const uint8_t *text, int64_t n, const uint32_t *tok, int64_t r)
{
    BgRec x;
    x.name_off = tok[4 * r];
    uint32_t e = x.name_off;
    while (e < n && !is_ws(text[e])) ++e;
    x.name_len = e - x.name_off;
    x.st = x.end = x.depth = 0;
    x.nfields = 1;
    if (parse_int(text, n, tok[4 * r + 1], &x.st)) {
        x.nfields = 2;
        if (parse_int(text, n, tok[4 * r + 2], &x.end)) {
            x.nfields = 3;
            if (parse_int(text, n, tok[4 * r + 3], &x.depth)) x.nfields = 4;
        }
    }
    return x;
}

__device__ __forceinline__ bool same_name(const uint8_t *a, uint32_t ao, uint32_t al, const uint8_t *b, uint32_t bo, uint32_t bl)
{
    if (al != bl) return false;
    for (uint32_t i = 0; i < al; ++i)
        if (a[ao + i] != b[bo + i]) return false;
    return true;
}

__device__ __forceinline__ uint32_t name_of(const uint8_t *text, int64_t n, const uint32_t *tok, int64_t r, uint32_t *len)
{
    const uint32_t o = tok[4 * r];
    uint32_t e = o;
    while (e < n && !is_ws(text[e])) ++e;
    *len = e - o;
    return o;
}

// contig segments of the flat arrays -> 64-element aligned layout of cornetto_cov_t
__global__ void bg_layout(const uint16_t *src, const int64_t *src_off, const int64_t *dst_off, const int32_t *len, int32_t n_ctg,
                          uint16_t *dst)
{
    // grid.y is limited to 65535: contigs are taken with a grid stride (read-level coverage sets have more)
    for (int c = blockIdx.y; c < n_ctg; c += gridDim.y) {
        const int64_t n = len[c];
        const uint16_t *s = src + src_off[c];
        uint16_t *d = dst + dst_off[c];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = s[i];
    }
}

// the token starts of d_text[0, n), in order
int tokenize(cornetto_accel_t *h, const uint8_t *d_text, int64_t n, int slot_tok, int slot_cnt, uint32_t **tok_out, int64_t *ntok)
{
    *ntok = 0;
    *tok_out = nullptr;
    if (n <= 0) return CORNETTO_OK;
    cnmarks::Marks mk;
    CN_TRY(cnmarks::count<tokstart_mask>(h, "bedgraph ingest", "tk_count", "tk_scan", d_text, n, slot_cnt, 0, &mk));
    CN_TRY(cnmarks::scatter<tokstart_mask>(h, "bedgraph ingest", "tk_scatter", d_text, n, mk, slot_tok, (size_t)mk.total, tok_out));
    *ntok = mk.total;
    return CORNETTO_OK;
}

// ---- compressed sources (cornetto_bgsrc_t): what both readers need to take BGZF blocks and to keep their carry on the device ----------------
enum { BG_BLOCK = 11 };   // the kind of a damaged block in cornetto_bgerr_t / cornetto_bgrunerr_t

// the bytes a source adds to its file (inflated bytes for a compressed one); false: not a source the feeds take
inline bool bgsrc_size(const cornetto_bgsrc_t *s, int64_t *n_new)
{
    *n_new = 0;
    if (!s) return true;
    if (s->n < 0 || s->n_blocks < 0 || s->n_blocks > 0x7fffffffLL || (s->n > 0 && (!s->text || s->n_blocks > 0)) || (s->n_blocks > 0 && (!s->comp || !s->blocks)))
        return false;
    for (int64_t i = 0; i < s->n_blocks; ++i) {
        const cornetto_bgzf_block_t &k = s->blocks[i];
        if (k.src < 0 || k.n_src < 0 || k.src > s->comp->cap - k.n_src || k.n_dst < 0 || k.n_dst > 65536) return false;
        *n_new += k.n_dst;
    }
    if (s->n > 0) *n_new = s->n;
    return true;
}
inline bool bgsrc_compressed(const cornetto_bgsrc_t *s) { return s && s->n_blocks > 0; }

// what a file carries from one feed to the next, on the device (a buffer of its own: cn_ws() does not keep what a slot held when it grows)
struct BgCarry {
    uint8_t *d = nullptr;
    size_t cap = 0;
    int64_t n = 0;
    bool on = false;     // the file has had a compressed source: its carry lives here, not in the host string
    int64_t blocks = 0;  // BGZF blocks of the file handed over so far
    void release() { if (d) (void)hipFree(d); d = nullptr; cap = 0; n = 0; }
};

inline int bg_carry_reserve(cornetto_accel_t *h, BgCarry &c, int64_t len)
{
    if ((size_t)len <= c.cap) return CORNETTO_OK;
    c.release();
    const size_t cap = (size_t)len + (size_t)len / 4 + 4096;
    if (hipMalloc((void **)&c.d, cap) != hipSuccess) { c.d = nullptr; return cn_fail(h, CORNETTO_E_NOMEM, "bedgraph ingest: device allocation of %zu bytes failed", cap); }
    c.cap = cap;
    return CORNETTO_OK;
}

// carry <- bytes [from, from + len) of the text workspace (another allocation: the ranges never overlap); queued on the handle's stream
inline int bg_carry_store(cornetto_accel_t *h, BgCarry &c, const uint8_t *d_from, int64_t len)
{
    CN_TRY(bg_carry_reserve(h, c, len));
    if (len > 0) CN_HIP(h, hipMemcpyAsync(c.d, d_from, (size_t)len, hipMemcpyDeviceToDevice, h->stream));
    c.n = len;
    return CORNETTO_OK;
}

// the file's first compressed source: what the host string carried goes to the device (the caller clears the string)
inline int bg_carry_from_host(cornetto_accel_t *h, BgCarry &c, const std::string &pend)
{
    CN_TRY(bg_carry_reserve(h, c, (int64_t)pend.size()));
    if (!pend.empty()) {
        CN_HIP(h, hipMemcpyAsync(c.d, pend.data(), pend.size(), hipMemcpyHostToDevice, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
    }
    c.n = (int64_t)pend.size();
    c.on = true;
    return CORNETTO_OK;
}

// Inflate the blocks of a compressed source behind the n_pend carried bytes of d_text (which has room for n_pend + the sum of n_dst).  *n_good: the
// inflated bytes in front of the first bad block (all of them when *first_bad is -1).
inline int bgsrc_inflate(cornetto_accel_t *h, const cornetto_bgsrc_t *s, uint8_t *d_text, int64_t n_pend, int64_t *first_bad, int64_t *n_good)
{
    for (int i = 0; i < 4; ++i) CN_HIP(h, hipStreamSynchronize(s->comp->q[i]));     // every slab is on the device
    std::vector<cornetto_bgzf_block_t> blk(s->blocks, s->blocks + s->n_blocks);
    int64_t at = n_pend;
    for (auto &k : blk) {
        k.dst = at;
        at += k.n_dst;
    }
    CN_TRY(cn_bgzf_inflate_raw(h, s->comp->d, d_text, blk.data(), s->n_blocks, first_bad));
    *n_good = (*first_bad >= 0 ? blk[(size_t)*first_bad].dst : at) - n_pend;
    return CORNETTO_OK;
}

// one byte of a device text, behind everything queued on the handle's stream
inline int bg_byte_at(cornetto_accel_t *h, const uint8_t *d_text, int64_t at, int *out)
{
    uint8_t *p = (uint8_t *)cn_pin(h, PIN_SMALL, 256);
    if (!p) return cn_fail(h, CORNETTO_E_NOMEM, "bedgraph ingest: workspace allocation failed");
    CN_HIP(h, hipMemcpyAsync(p + 248, d_text + at, 1, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    *out = p[248];
    return CORNETTO_OK;
}

// The contig names of a feed's contig starts, packed on the device and copied once: a block of 64 lanes per name.  brk[k] holds the name's
// offset and length in the text (.z / .w in the per-base reader's list, .y / .z in the run reader's); both lie inside the text (name_of()).
__global__ __launch_bounds__(64) void bg_names(const uint8_t *__restrict__ text, const uint4 *__restrict__ brk, uint32_t n, int runs, const uint32_t *__restrict__ to,
                                                uint8_t *__restrict__ pack)
{
    const uint32_t k = blockIdx.x;
    if (k >= n) return;
    const uint4 x = brk[k];
    const uint32_t off = runs ? x.y : x.z, len = runs ? x.z : x.w;
    for (uint32_t i = threadIdx.x; i < len; i += 64) pack[to[k] + i] = text[off + i];
}

int bg_fetch_names(cornetto_accel_t *h, const uint8_t *d_text, const uint4 *d_brk, const std::vector<uint4> &brk, int runs, std::vector<std::string> *names)
{
    names->assign(brk.size(), std::string());
    const uint32_t nb = (uint32_t)brk.size();
    if (!nb) return CORNETTO_OK;
    std::vector<uint32_t> to(nb);
    size_t total = 0;
    for (uint32_t k = 0; k < nb; ++k) {
        to[k] = (uint32_t)total;
        total += runs ? brk[k].z : brk[k].w;
    }
    if (total == 0) return CORNETTO_OK;
    if (total > 0xF0000000ull) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "bedgraph ingest: the contig names of one feed have more than 3.75 GiB");
    const size_t head = ((size_t)nb * 4 + 15) & ~(size_t)15;
    uint8_t *d_pack = (uint8_t *)cn_ws(h, WS_BZ_PACK, head + total);
    if (!d_pack) return cn_fail(h, CORNETTO_E_NOMEM, "bedgraph ingest: workspace allocation failed");
    std::string pack(total, '\0');
    CN_HIP(h, hipMemcpyAsync(d_pack, to.data(), (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
    CN_LAUNCH(h, "bg_names", bg_names<<<dim3(nb), dim3(64), 0, h->stream>>>(d_text, d_brk, nb, runs, reinterpret_cast<const uint32_t *>(d_pack), d_pack + head));
    CN_HIP(h, hipMemcpyAsync(&pack[0], d_pack + head, total, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < nb; ++k) (*names)[k].assign(pack, to[k], runs ? brk[k].z : brk[k].w);
    return CORNETTO_OK;
}

// the contigs of two flat depth arrays ([src_off[i], src_off[i] + lens[i]) of d_a / d_b) -> the arrays of `c` (c->n and whatever else the caller knows
// are set; the tables, the totals and the device memory are filled here).  On failure `c` is released.
int bg_cov_layout(cornetto_accel_t *h, const char *who, cornetto_cov_t *c, const uint16_t *d_a, const uint16_t *d_b, const std::vector<int64_t> &src_off,
                  const std::vector<int64_t> &lens)
{
    const int32_t nc = (int32_t)src_off.size();
    int64_t pos = 0;
    for (int32_t i = 0; i < nc; ++i) {
        if (lens[i] > INT32_MAX) { delete c; return cn_fail(h, CORNETTO_E_UNSUPPORTED, "%s: contig %d has more than 2^31-1 positions", who, i); }
        c->off.push_back(pos);
        c->len.push_back((int32_t)lens[i]);
        c->total += lens[i];
        pos = cn_align_up(pos + lens[i], 64);
    }
    const size_t bytes = (size_t)(pos + 256) * sizeof(uint16_t);
    const size_t ntab = (size_t)(nc > 0 ? nc : 1);
    int64_t *d_src = nullptr;
    if (hipMalloc(&c->owned_d, bytes) != hipSuccess || hipMalloc(&c->owned_q, bytes) != hipSuccess ||
        hipMalloc((void **)&c->d_off, ntab * 8) != hipSuccess || hipMalloc((void **)&c->d_len, ntab * 4) != hipSuccess ||
        hipMalloc((void **)&d_src, ntab * 8) != hipSuccess) {
        if (d_src) (void)hipFree(d_src);
        cornetto_cov_free(h, c);
        return cn_fail(h, CORNETTO_E_NOMEM, "%s: device allocation failed", who);
    }
    c->d_depth = (const uint16_t *)c->owned_d;
    c->d_mq = (const uint16_t *)c->owned_q;
    hipError_t e = hipMemsetAsync(c->owned_d, 0, bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->owned_q, 0, bytes, h->stream);
    if (nc) {
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_off, c->off.data(), (size_t)nc * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_len, c->len.data(), (size_t)nc * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_src, src_off.data(), (size_t)nc * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            bg_layout<<<dim3(64, (unsigned)std::min<int32_t>(nc, 32768)), dim3(256), 0, h->stream>>>(d_a, d_src, c->d_off, c->d_len, nc, (uint16_t *)c->owned_d);
            bg_layout<<<dim3(64, (unsigned)std::min<int32_t>(nc, 32768)), dim3(256), 0, h->stream>>>(d_b, d_src, c->d_off, c->d_len, nc, (uint16_t *)c->owned_q);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_src);
    if (e != hipSuccess) {
        cornetto_cov_free(h, c);
        return cn_fail(h, CORNETTO_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return CORNETTO_OK;
}

}  // namespace
