// ktrio.hip — `cornetto trioeval`: the k-mer table of `qv` with a parental tag per key (cornetto_kset_add_tag), and the switch / Hamming counts of
// a phased assembly against it (cornetto_kset_phase).  include/cornetto_accel.h states the rule; kqv.hpp has the k-mers and the tagged table,
// ktrio.hpp the ordered pass (and tools/sim/ktrio_sim.cc runs both on the CPU under the host sanitizers: the argument for the bounds below).
// Not in the reference: its protocol runs `yak trioeval` here.  All kernels run on the handle's stream; kernel boundaries are the only ordering.
//   kt_insert   kq_insert with kq_insert_tag(): an agent-scope compare-and-swap per probe and, for a key that is there without this call's tag,
//               one agent-scope fetch-or.  Only values returned by those atomics decide anything: no plain load of the table in this kernel;
//   kt_mark     kq_query's extraction and a tagged lookup with plain loads (the table is complete at the kernel boundary).  kmers, pat and mat are
//               counted over the wave by ballots, one 64-bit atomic add each per wave (a wave lies in one tile, a tile in one contig).  A marker
//               sets its bit with an atomic OR in the pat or the mat bitmap (tiles * KQ_TILE bits each, kq_bit(); the call zeroed both).  A
//               thread owns the k-mers that END in its run, so the first k - 1 positions' worth of a tile's bits are written by the workgroup
//               behind it: a tile's words are complete only at the kernel boundary, which is why the ordered pass is another kernel;
//   kt_tile     a wave per tile, lane l = word l of the tile's 64 words of either bitmap: pairs inside the word from the two words, the type in
//               front of each word from a wave scan (6 __shfl_up steps), the packed pair counts summed over the wave, at most four atomic adds
//               by lane 0 into the contig's counters; the tile's byte first | last << 2;
//   kt_seam     a wave per tile.  It leaves at once if its tile has no marker or is its contig's first tile.  Otherwise it reads the bytes of the
//               64 tiles in front of it per round, never in front of the contig's first tile, ballots on last != none, takes the nearest and
//               adds the one pair (that last, own first).  The walk of a wave ends at the nearest tile in front that has a marker, or at the
//               contig's first tile when there is none; every tile strictly between is marker-free, and so starts no walk.  The stretches walked
//               by two waves are therefore disjoint — each lies between two consecutive marker tiles of one contig, or in front of a contig's
//               first one — and their lengths sum to at most the number of tiles, rounded up to a round per walking wave: linear in the tiles.
//               No walk reads in front of t0, so no pair spans two contigs, and a walk that finds nothing adds nothing: the contig's first
//               marker has no pair.
// Bounds: tab[slot] with slot < slots; seq[i] with 0 <= i < len of the tile's contig; a bit of tile t lies in words [t * 64, (t + 1) * 64) of a
// bitmap of n_tiles * 64 words; tb[t] with t0 <= t < n_tiles; cnt[7 * c + j] with c < n contigs, j < 7.
#include <vector>

#include "common.hpp"
#include "kqv.hpp"
#include "kset.hpp"
#include "ktrio.hpp"

namespace {

constexpr int KT_TILES_PER_BLOCK = 4;   // kt_tile, kt_seam: 256 threads, a wave a tile

__device__ __forceinline__ uint32_t kt_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ void __launch_bounds__(KQ_THREADS) kt_insert_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                              const int2 *__restrict__ tiles, int k, uint64_t *tab, uint64_t slots, uint64_t tag, unsigned long long *stat)
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
    auto fetch_or = [](uint64_t *p, uint64_t bits) -> uint64_t {
        return (uint64_t)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long *>(p), (unsigned long long)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto stop = [stat]() -> bool { return __hip_atomic_load(stat + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; };
    uint32_t n_pos = 0, n_new = 0;
    bool full = false;
    for (int r = 0; r < KQ_RUN; ++r) {   // (the same trip count in every lane: the ballots see the whole wave)
        int64_t pos;
        uint64_t key;
        const bool has = kq_step(seq, b0, b1, r, s, k, pos, key);
        const int res = has ? kq_insert_tag(tab, slots, key, tag, cas, fetch_or, stop) : KQ_PRESENT;
        n_pos += kt_count(has && res != KQ_FULL);
        n_new += kt_count(res == KQ_NEW);
        full |= res == KQ_FULL;
    }
    if (full) (void)atomicOr(stat + 2, 1ull);
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) (void)atomicAdd(stat + 0, (unsigned long long)n_pos);
        if (n_new) (void)atomicAdd(stat + 1, (unsigned long long)n_new);
    }
}

__global__ void __launch_bounds__(KQ_THREADS) kt_mark_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                            const int2 *__restrict__ tiles, int k, const uint64_t *__restrict__ tab, uint64_t slots,
                                                            unsigned long long *cnt, unsigned long long *pat, unsigned long long *mat)
{
    const int2 t = tiles[blockIdx.x];
    const uint8_t *seq = bases + off[t.x];
    int64_t b0, b1;
    kq_bounds(t.y, (int)threadIdx.x, len[t.x], b0, b1);
    KqRoll s = {0, 0, 0};
    if (b0 < b1) s = kq_lead(seq, b0, k);
    const int64_t tile0 = (int64_t)blockIdx.x - t.y / KQ_TILE;   // the contig's first tile
    uint32_t n_pos = 0, n_pat = 0, n_mat = 0;
    for (int r = 0; r < KQ_RUN; ++r) {
        int64_t pos;
        uint64_t key;
        const bool has = kq_step(seq, b0, b1, r, s, k, pos, key);
        const int tag = has ? kq_lookup_tag(tab, slots, key) : 0;
        if (tag == KT_PAT || tag == KT_MAT) {
            int64_t word;
            uint64_t mask;
            kq_bit(tile0, pos, word, mask);
            (void)atomicOr((tag == KT_PAT ? pat : mat) + word, (unsigned long long)mask);
        }
        n_pos += kt_count(has);
        n_pat += kt_count(tag == KT_PAT);
        n_mat += kt_count(tag == KT_MAT);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *c = cnt + KT_COUNTS * (int64_t)t.x;
        if (n_pos) (void)atomicAdd(c + 0, (unsigned long long)n_pos);
        if (n_pat) (void)atomicAdd(c + 1, (unsigned long long)n_pat);
        if (n_mat) (void)atomicAdd(c + 2, (unsigned long long)n_mat);
    }
}

__global__ void __launch_bounds__(64 * KT_TILES_PER_BLOCK) kt_tile_kernel(const unsigned long long *__restrict__ pat, const unsigned long long *__restrict__ mat,
                                                                         const int2 *__restrict__ tiles, int64_t nt, unsigned long long *cnt, uint8_t *__restrict__ tb)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * KT_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (t >= nt) return;   // (the whole wave)
    const uint64_t p = pat[t * KT_WORDS + lane], m = mat[t * KT_WORDS + lane];
    int incl = kt_last(p, m);   // -> the type of the last marker at or in front of this word, in the tile
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl = kt_op(o, incl);
    }
    int in = __shfl_up(incl, 1);
    if (lane == 0) in = KT_NONE;
    unsigned long long pairs = kt_word(p, m, in);
    for (int d = 32; d; d >>= 1) pairs += __shfl_xor(pairs, d);
    const unsigned long long has = __ballot((p | m) != 0);
    const int first = has ? __shfl(kt_first(p, m), __ffsll(has) - 1) : KT_NONE;
    const int last = __shfl(incl, 63);
    if (lane == 0) {
        tb[t] = kt_tile_byte(first, last);
        unsigned long long *c = cnt + KT_COUNTS * (int64_t)tiles[t].x + 3;
        for (int i = 0; i < 4; ++i) {
            const unsigned long long v = (pairs >> (16 * i)) & 0xFFFF;
            if (v) (void)atomicAdd(c + i, v);
        }
    }
}

__global__ void __launch_bounds__(64 * KT_TILES_PER_BLOCK) kt_seam_kernel(const uint8_t *__restrict__ tb, const int2 *__restrict__ tiles, int64_t nt, unsigned long long *cnt)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * KT_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (t >= nt) return;
    const int2 tl = tiles[t];
    const int64_t t0 = t - tl.y / KQ_TILE;   // the contig's first tile
    const int first = kt_byte_first(tb[t]);
    if (first == KT_NONE || t == t0) return;
    for (int64_t hi = t; hi > t0; hi -= KT_WORDS) {   // at most ceil((t - t0) / 64) rounds
        const int v = kt_seam_look(tb, t0, hi, lane);
        const unsigned long long b = __ballot(v != KT_NONE);
        if (!b) continue;
        const int last = __shfl(v, __ffsll(b) - 1);   // the lowest lane looks at the nearest tile
        if (lane == 0) (void)atomicAdd(cnt + KT_COUNTS * (int64_t)tl.x + 3 + kt_pair(last, first), 1ull);
        return;
    }
}

}  // namespace

extern "C" {

int cornetto_kset_add_tag(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a, int32_t tag)
{
    if (!h || !s || !a || (tag != CORNETTO_TRIO_PAT && tag != CORNETTO_TRIO_MAT)) return cn_fail(h, CORNETTO_E_ARG, "kset_add_tag: bad argument (the tag is 1, pat, or 2, mat)");
    if (s->counted) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_add_tag: the set is counted (kset_count); it takes no keys without a count");
    if (s->mode == KSET_PLAIN) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_add_tag: the set is plain (kset_add); a set is either plain or tagged");
    if (s->dead) return cn_fail(h, CORNETTO_E_NOMEM, "kset_add_tag: the table of %lld slots has overflowed; the set is unusable", (long long)s->slots);
    s->mode = KSET_TAGGED;
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t nt = kq_tiles(h, s, a);
    if (nt < 0) return (int)nt;
    unsigned long long *p_stat = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!p_stat) return cn_fail(h, CORNETTO_E_NOMEM, "kset_add_tag: host allocation failed");
    if (nt > 0)
        CN_LAUNCH(h, "kt_insert", kt_insert_kernel<<<dim3((unsigned)nt), dim3(KQ_THREADS), 0, h->stream>>>(a->d_bases, a->d_off, a->d_len, s->d_tiles, s->k, s->d_tab,
                                                                                                          (uint64_t)s->slots, (uint64_t)tag, s->d_stat));
    CN_HIP(h, hipMemcpyAsync(p_stat, s->d_stat, 24, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    s->stats[0] = (int64_t)p_stat[0];
    s->stats[1] = (int64_t)p_stat[1];
    if (p_stat[2]) {
        s->dead = true;
        return cn_fail(h, CORNETTO_E_NOMEM, "kset_add_tag: the table of %lld slots overflowed (%lld distinct k-mers are in it); the set is unusable", (long long)s->slots,
                       (long long)s->stats[1]);
    }
    return CORNETTO_OK;
}

int cornetto_kset_phase(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a, int64_t *counts)
{
    if (!h || !s || !a || (a->n > 0 && !counts)) return cn_fail(h, CORNETTO_E_ARG, "kset_phase: bad argument");
    if (s->mode == KSET_COUNTED) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_phase: the set is counted and not sealed yet (kset_seal)");
    if (s->mode == KSET_PLAIN) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_phase: the set is plain; its query is kset_query");
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_phase: the set is unusable, its table has overflowed");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t nt = kq_tiles(h, s, a);
    if (nt < 0) return (int)nt;
    const size_t n = (size_t)a->n;
    if (nt > 0) {
        const size_t nw = (size_t)nt * KT_WORDS;
        unsigned long long *d_cnt = (unsigned long long *)cn_ws(h, WS_KT_CNT, KT_COUNTS * n * 8);
        uint8_t *map = (uint8_t *)cn_ws(h, WS_KT_MAP, 2 * nw * 8 + (size_t)nt);   // the pat bitmap, the mat bitmap, the tile bytes
        if (!d_cnt || !map) return cn_fail(h, CORNETTO_E_NOMEM, "kset_phase: workspace allocation failed (%lld bytes)", (long long)(2 * nw * 8 + (size_t)nt));
        unsigned long long *d_pat = (unsigned long long *)map, *d_mat = d_pat + nw;
        uint8_t *d_tb = map + 2 * nw * 8;   // (every tile's byte is written by kt_tile)
        CN_HIP(h, hipMemsetAsync(d_cnt, 0, KT_COUNTS * n * 8, h->stream));
        CN_HIP(h, hipMemsetAsync(d_pat, 0, 2 * nw * 8, h->stream));
        const unsigned nb = (unsigned)((nt + KT_TILES_PER_BLOCK - 1) / KT_TILES_PER_BLOCK);
        CN_LAUNCH(h, "kt_mark", kt_mark_kernel<<<dim3((unsigned)nt), dim3(KQ_THREADS), 0, h->stream>>>(a->d_bases, a->d_off, a->d_len, s->d_tiles, s->k, s->d_tab,
                                                                                                      (uint64_t)s->slots, d_cnt, d_pat, d_mat));
        CN_LAUNCH(h, "kt_tile", kt_tile_kernel<<<dim3(nb), dim3(64 * KT_TILES_PER_BLOCK), 0, h->stream>>>(d_pat, d_mat, s->d_tiles, nt, d_cnt, d_tb));
        CN_LAUNCH(h, "kt_seam", kt_seam_kernel<<<dim3(nb), dim3(64 * KT_TILES_PER_BLOCK), 0, h->stream>>>(d_tb, s->d_tiles, nt, d_cnt));
        std::vector<unsigned long long> cnt(KT_COUNTS * n);
        CN_HIP(h, hipMemcpyAsync(cnt.data(), d_cnt, KT_COUNTS * n * 8, hipMemcpyDeviceToHost, h->stream));
        CN_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < KT_COUNTS * n; ++i) counts[i] = (int64_t)cnt[i];
    } else {
        for (size_t i = 0; i < KT_COUNTS * n; ++i) counts[i] = 0;
    }
    cn_timing_end(h);
    s->mode = KSET_TAGGED;
    return CORNETTO_OK;
}

}  // extern "C"
