// kqv.hip — `cornetto qv`: a set of canonical k-mers resident in HBM (cornetto_kset_*), filled from truth assemblies and probed with every
// position of a query assembly.  include/cornetto_accel.h states the rule, kqv.hpp has the arithmetic (and tools/sim/kqv_sim.cc runs it on the
// CPU under the host sanitizers: the argument for the bounds below).  Not in the reference: its protocol runs `yak count` / `yak qv` here.
//   kq_insert     a workgroup per tile of KQ_TILE bases, a thread a run of KQ_RUN bases: the k-mers that end in the run go into the
//                 open-addressing table with an agent-scope compare-and-swap per probe — only the value the CAS returns ends a probe, no
//                 plain load of the table in this kernel (the XCDs' L2s are not coherent for those).  New keys and inserted positions are
//                 counted over the wave by ballots, one atomic add each per wave.  A probe takes at most `slots` steps, then raises the
//                 overflow word, which the other lanes poll every 1024 steps;
//   kq_query      the same extraction; plain loads of the table (complete at the kernel boundary); k-mers and missing k-mers counted over the
//                 wave by ballots, one 64-bit atomic add each per wave (a wave lies in one tile, a tile in one contig); with runs, an
//                 atomic OR of the position's bit into a bitmap the call zeroed;
//   kq_run_count, kq_run_emit   the bitmap's runs of set bits as rows {ctg, i0, i1 + k}: starts counted per word, scanned (scan.hpp), starts
//                 and ends written by rank; then the merge of ivlmerge.hpp with distance 0 (an interval that starts at or before the largest
//                 finish so far in its contig is merged: overlapping and book-ended spans, which is the rule).
// Bounds: tab[slot] with slot < slots (kq_home() < slots, kq_next() wraps); seq[i] with 0 <= i < len of the tile's contig; a bit of tile t lies
// in words [t * KQ_TILE / 64, (t + 1) * KQ_TILE / 64) of a bitmap of n_tiles * KQ_TILE bits; rows[r] with r < the scanned total of the same bitmap.
#include <new>

#include "common.hpp"
#include "ivlmerge.hpp"
#include "kqv.hpp"
#include "kset.hpp"
#include "scan.hpp"
#include "tiles.hpp"

namespace {

__device__ __forceinline__ uint32_t kq_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ void __launch_bounds__(KQ_THREADS) kq_insert_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                              const int2 *__restrict__ tiles, int k, uint64_t *tab, uint64_t slots, unsigned long long *stat)
{
    const int2 t = tiles[blockIdx.x];
    const uint8_t *seq = bases + off[t.x];
    int64_t b0, b1;
    kq_bounds(t.y, (int)threadIdx.x, len[t.x], b0, b1);
    KqRoll s = {0, 0, 0};
    if (b0 < b1) s = kq_lead(seq, b0, k);
    auto cas = [](uint64_t *p, uint64_t expect, uint64_t val) -> uint64_t {
        unsigned long long e = expect;
        (void)__hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long *>(p), &e, (unsigned long long)val, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        return (uint64_t)e;
    };
    auto stop = [stat]() -> bool { return __hip_atomic_load(stat + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; };
    uint32_t n_pos = 0, n_new = 0;
    bool full = false;
    for (int r = 0; r < KQ_RUN; ++r) {   // (the same trip count in every lane: the ballots see the whole wave)
        int64_t pos;
        uint64_t key;
        const bool has = kq_step(seq, b0, b1, r, s, k, pos, key);
        const int res = has ? kq_insert(tab, slots, key, cas, stop) : KQ_PRESENT;
        n_pos += kq_count(has && res != KQ_FULL);
        n_new += kq_count(res == KQ_NEW);
        full |= res == KQ_FULL;
    }
    if (full) (void)atomicOr(stat + 2, 1ull);
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) (void)atomicAdd(stat + 0, (unsigned long long)n_pos);
        if (n_new) (void)atomicAdd(stat + 1, (unsigned long long)n_new);
    }
}

__global__ void __launch_bounds__(KQ_THREADS) kq_query_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                             const int2 *__restrict__ tiles, int k, const uint64_t *__restrict__ tab, uint64_t slots,
                                                             unsigned long long *cnt, unsigned long long *bits)
{
    const int2 t = tiles[blockIdx.x];
    const uint8_t *seq = bases + off[t.x];
    int64_t b0, b1;
    kq_bounds(t.y, (int)threadIdx.x, len[t.x], b0, b1);
    KqRoll s = {0, 0, 0};
    if (b0 < b1) s = kq_lead(seq, b0, k);
    const int64_t tile0 = (int64_t)blockIdx.x - t.y / KQ_TILE;   // the contig's first tile
    uint32_t n_pos = 0, n_miss = 0;
    for (int r = 0; r < KQ_RUN; ++r) {
        int64_t pos;
        uint64_t key;
        const bool has = kq_step(seq, b0, b1, r, s, k, pos, key);
        const bool miss = has && !kq_lookup(tab, slots, key);
        if (miss && bits) {
            int64_t word;
            uint64_t mask;
            kq_bit(tile0, pos, word, mask);
            (void)atomicOr(bits + word, (unsigned long long)mask);
        }
        n_pos += kq_count(has);
        n_miss += kq_count(miss);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) (void)atomicAdd(cnt + 2 * (int64_t)t.x, (unsigned long long)n_pos);
        if (n_miss) (void)atomicAdd(cnt + 2 * (int64_t)t.x + 1, (unsigned long long)n_miss);
    }
}

__global__ void __launch_bounds__(256) kq_run_count(const unsigned long long *__restrict__ bits, int64_t nw, uint32_t *__restrict__ cnt)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;
    cnt[w] = (uint32_t)__popcll(kq_starts(bits[w], w ? bits[w - 1] >> 63 : 0));
}

__global__ void __launch_bounds__(256) kq_run_emit(const unsigned long long *__restrict__ bits, int64_t nw, const uint32_t *__restrict__ rank, const int2 *__restrict__ tiles,
                                                  int k, cornetto_ivl_t *__restrict__ rows)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;
    const uint64_t v = bits[w];
    if (!v) return;
    const uint64_t prev = w ? bits[w - 1] >> 63 : 0, next = w + 1 < nw ? bits[w + 1] : 0;
    const int2 t = tiles[w / (KQ_TILE / 64)];
    const int32_t p0 = t.y + (int32_t)(w % (KQ_TILE / 64)) * 64;
    uint32_t r = rank[w];
    for (uint64_t m = kq_starts(v, prev); m; m &= m - 1, ++r) {
        rows[r].ctg = t.x;
        rows[r].start = p0 + (__ffsll((unsigned long long)m) - 1);
    }
    r = kq_end_rank(rank[w], v, prev);
    for (uint64_t m = kq_ends(v, next); m; m &= m - 1, ++r) rows[r].finish = p0 + (__ffsll((unsigned long long)m) - 1) + k;
}

}  // namespace

extern "C" {

int cornetto_kset_open(cornetto_accel_t *h, int32_t k, int64_t slots, cornetto_kset_t **out) { return kq_open(h, "kset_open", k, slots, 0, out); }

void cornetto_kset_free(cornetto_accel_t *h, cornetto_kset_t *s)
{
    if (!s) return;
    if (h) (void)hipSetDevice(h->device);
    if (s->d_tab) (void)hipFree(s->d_tab);
    if (s->d_stat) (void)hipFree(s->d_stat);
    if (s->d_cnt) (void)hipFree(s->d_cnt);
    if (s->d_cop) (void)hipFree(s->d_cop);
    if (s->d_tiles) (void)hipFree(s->d_tiles);
    s->pref.release();
    delete s;
}

void cornetto_kset_stats(const cornetto_kset_t *s, int64_t *stats)
{
    if (!s || !stats) return;
    for (int i = 0; i < 3; ++i) stats[i] = s->stats[i];
}

int cornetto_kset_add(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *truth)
{
    if (!h || !s || !truth) return cn_fail(h, CORNETTO_E_ARG, "kset_add: bad argument");
    if (s->counted) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_add: the set is counted (kset_count); it takes no keys without a count");
    if (s->mode == KSET_TAGGED) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_add: the set is tagged (kset_add_tag); a set is either plain or tagged");
    if (s->dead) return cn_fail(h, CORNETTO_E_NOMEM, "kset_add: the table of %lld slots has overflowed; the set is unusable", (long long)s->slots);
    s->mode = KSET_PLAIN;
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t nt = kq_tiles(h, s, truth);
    if (nt < 0) return (int)nt;
    unsigned long long *p_stat = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!p_stat) return cn_fail(h, CORNETTO_E_NOMEM, "kset_add: host allocation failed");
    if (nt > 0)
        CN_LAUNCH(h, "kq_insert", kq_insert_kernel<<<dim3((unsigned)nt), dim3(KQ_THREADS), 0, h->stream>>>(truth->d_bases, truth->d_off, truth->d_len, s->d_tiles, s->k,
                                                                                                          s->d_tab, (uint64_t)s->slots, s->d_stat));
    CN_HIP(h, hipMemcpyAsync(p_stat, s->d_stat, 24, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    s->stats[0] = (int64_t)p_stat[0];
    s->stats[1] = (int64_t)p_stat[1];
    if (p_stat[2]) {
        s->dead = true;
        return cn_fail(h, CORNETTO_E_NOMEM, "kset_add: the table of %lld slots overflowed (%lld distinct k-mers are in it); the set is unusable", (long long)s->slots,
                       (long long)s->stats[1]);
    }
    return CORNETTO_OK;
}

int cornetto_kset_query(cornetto_accel_t *h, const cornetto_kset_t *cs, const cornetto_asm_t *a, int64_t *kmers, int64_t *missing, cornetto_ivl_t **runs, int64_t *n_runs)
{
    if (!h || !cs || !a || (a->n > 0 && (!kmers || !missing)) || (!runs != !n_runs)) return cn_fail(h, CORNETTO_E_ARG, "kset_query: bad argument");
    cornetto_kset_t *s = const_cast<cornetto_kset_t *>(cs);   // (its tile table is scratch)
    if (runs) {
        *runs = nullptr;
        *n_runs = 0;
    }
    if (s->mode == KSET_COUNTED) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_query: the set is counted and not sealed yet (kset_seal)");
    if (s->mode == KSET_TAGGED) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_query: the set is tagged; its query is kset_phase");
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_query: the set is unusable, its table has overflowed");
    // the runs are placed by 32-bit ranks: at most one run per two positions and one more per contig
    if (runs && a->total / 2 + a->n > 0xFFFFFFFFll)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_query: %lld bases in %d contigs could hold more than 2^32-1 runs", (long long)a->total, (int)a->n);
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t nt = kq_tiles(h, s, a);
    if (nt < 0) return (int)nt;
    const size_t n = (size_t)a->n;
    cornetto_ivl_t *o = nullptr;
    int64_t m = 0;
    if (nt > 0) {
        unsigned long long *d_cnt = (unsigned long long *)cn_ws(h, WS_KQ_CNT, 2 * n * 8);
        unsigned long long *p_cnt = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
        if (!d_cnt || !p_cnt) return cn_fail(h, CORNETTO_E_NOMEM, "kset_query: workspace allocation failed");
        CN_HIP(h, hipMemsetAsync(d_cnt, 0, 2 * n * 8, h->stream));
        const int64_t nw = nt * (KQ_TILE / 64);
        unsigned long long *d_bits = nullptr, *d_total = nullptr;
        uint32_t *d_rc = nullptr, *d_rank = nullptr;
        if (runs) {   // bitmap [nw] u64, starts per word [nw] u32, their ranks [nw] u32, the total
            uint8_t *map = (uint8_t *)cn_ws(h, WS_KQ_MAP, (size_t)nw * 16 + 16);
            if (!map) return cn_fail(h, CORNETTO_E_NOMEM, "kset_query: workspace allocation failed (%lld bytes)", (long long)nw * 16 + 16);
            d_bits = (unsigned long long *)map;
            d_total = d_bits + nw;
            d_rc = (uint32_t *)(d_total + 1);
            d_rank = d_rc + nw;
            CN_HIP(h, hipMemsetAsync(d_bits, 0, (size_t)nw * 8 + 8, h->stream));
        }
        CN_LAUNCH(h, "kq_query", kq_query_kernel<<<dim3((unsigned)nt), dim3(KQ_THREADS), 0, h->stream>>>(a->d_bases, a->d_off, a->d_len, s->d_tiles, s->k, s->d_tab,
                                                                                                        (uint64_t)s->slots, d_cnt, d_bits));
        std::vector<unsigned long long> cnt(2 * n);
        CN_HIP(h, hipMemcpyAsync(cnt.data(), d_cnt, 2 * n * 8, hipMemcpyDeviceToHost, h->stream));
        if (runs) {
            CN_LAUNCH(h, "kq_run_count", kq_run_count<<<dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream>>>(d_bits, nw, d_rc));
            CN_TRY(cnscan::exclusive_u32(h, "kq_run_scan", d_rc, nw, 1, d_rank, d_total));
            CN_HIP(h, hipMemcpyAsync(p_cnt, d_total, 8, hipMemcpyDeviceToHost, h->stream));
        }
        CN_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t c = 0; c < n; ++c) {
            kmers[c] = (int64_t)cnt[2 * c];
            missing[c] = (int64_t)cnt[2 * c + 1];
        }
        const int64_t nr = runs ? (int64_t)p_cnt[0] : 0;
        if (nr > 0) {   // rows [nr], merged rows [nr], the merge's workspace, its count
            const size_t rows_bytes = ((size_t)nr * sizeof(cornetto_ivl_t) + 15) & ~(size_t)15;
            uint8_t *ws = (uint8_t *)cn_ws(h, WS_KQ_ROWS, 2 * rows_bytes + cnivl::ws_bytes((size_t)nr) + 16);
            if (!ws) return cn_fail(h, CORNETTO_E_NOMEM, "kset_query: workspace allocation failed");
            cornetto_ivl_t *d_rows = (cornetto_ivl_t *)ws, *d_out = (cornetto_ivl_t *)(ws + rows_bytes);
            unsigned long long *d_m = (unsigned long long *)(ws + 2 * rows_bytes);
            uint8_t *mws = ws + 2 * rows_bytes + 16;
            CN_LAUNCH(h, "kq_run_emit", kq_run_emit<<<dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream>>>(d_bits, nw, d_rank, s->d_tiles, s->k, d_rows));
            CN_TRY(cnivl::merge(h, "kq_run_merge", d_rows, nr, 0, mws, d_out, d_m));
            CN_HIP(h, hipMemcpyAsync(p_cnt, d_m, 8, hipMemcpyDeviceToHost, h->stream));
            CN_HIP(h, hipStreamSynchronize(h->stream));
            m = (int64_t)p_cnt[0];
            o = (cornetto_ivl_t *)cn_result_alloc(((size_t)m ? (size_t)m : 1) * sizeof(cornetto_ivl_t));
            if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "kset_query: host allocation failed");
            if (m > 0 && (hipMemcpyAsync(o, d_out, (size_t)m * sizeof(cornetto_ivl_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                          hipStreamSynchronize(h->stream) != hipSuccess)) {
                cornetto_free(o);
                return cn_fail(h, CORNETTO_E_HIP, "kset_query: copy back failed");
            }
        }
    } else {
        for (size_t c = 0; c < n; ++c) kmers[c] = missing[c] = 0;
    }
    cn_timing_end(h);
    if (runs) {
        if (!o) o = (cornetto_ivl_t *)cn_result_alloc(sizeof(cornetto_ivl_t));
        if (!o) return cn_fail(h, CORNETTO_E_NOMEM, "kset_query: host allocation failed");
        *runs = o;
        *n_runs = m;
    }
    return CORNETTO_OK;
}

}  // extern "C"
