// kcount.hip — the counted k-mer set of `cornetto qv -r` and `cornetto trioeval --pat-reads / --mat-reads`: the table of kqv.hip with a count per
// key and channel, its histogram, and the seal that turns counts and thresholds into the plain or the tagged set the kernels of kqv.hip and
// ktrio.hip probe.  include/cornetto_accel.h states the rule, kqv.hpp has the arithmetic and the two proofs (the count never wraps: kq_bump();
// the tombstone equals no key: KQ_TOMB), and tools/sim/kcount_sim.cc runs it on the CPU under the host sanitizers: the argument for the bounds.
// Not in the reference: its protocol runs `yak count` on the parental reads here.  All kernels run on the handle's stream; kernel boundaries are
// the only ordering between them.
//   kq_count   lanes are dealt runs, not records: reads are often 150 bases, and a workgroup per record's 4096-base tile (kq_insert) would leave
//              10 of 256 lanes busy on them.  first[] is the prefix of ceil(len / KQ_RUN) over the batch's records (tiles.hpp); thread g finds
//              its record by bisection in it and does kq_lead() + KQ_RUN steps inside that record only, so a wave may span records — counting
//              has no per-record output.  Per k-mer: kq_insert's walk (an agent-scope compare-and-swap per probe; only the value it returns ends a
//              probe) in the variant that yields the slot, then kq_bump(): one relaxed agent-scope load of count[ch * slots + slot] and, while
//              it reads below the cap, one no-return agent-scope atomic add.  Positions and new keys are counted over the wave by ballots, one
//              atomic add each per wave.  A probe takes at most `slots` steps, then raises the overflow word, which the other lanes poll every
//              1024 steps: a table too small is a status, never a hang;
//   kq_hist    grid-stride over the slots of one channel; a workgroup bins min(count, BINS - 1) of the non-zero counts into 1024 uint32_t of LDS
//              (a workgroup sees at most ceil(slots / 256 / blocks) * 256 < 2^32 slots) and adds its non-zero bins with 64-bit atomics into
//              WS_KC_HIST, which the call zeroed.  Plain loads of the counts: complete at the kernel boundary;
//   kq_seal    a thread per slot, plain loads and stores (complete at the kernel boundary; each thread touches its own slot only): an occupied
//              slot becomes kq_seal_word() — the key, the key with its tag, or the tombstone.  The solid keys of either channel are counted over
//              the wave by ballots, one atomic add each per wave.
//   kq_copies, kq_spectrum   the copies of an assembly beside the counts of a one-channel set, and the 6 x 1024 spectrum of the two (`qv -r
//              --completeness / --spectra-cn`): described in front of the kernels; kqv.hpp has the byte packing and the termination argument of
//              kq_copy_bump(), tools/sim/kspec_sim.cc runs both on the CPU.  Bounds: cop[slot >> 2] with slot < slots in ceil(slots / 4) words;
//              cells[a * 1024 + bin] with a <= 5 and bin < 1024; out[i] with i < 6 * 1024 + 2.
// Bounds: first[c] with c <= n; seq[i] with 0 <= i < len of the run's record (kq_deal(): b1 <= len; kq_lead() starts at max(b0 - k + 1, 0));
// tab[slot] and cnt[ch * slots + slot] with slot < slots (kq_home() < slots, kq_next() wraps) and ch < channels; hist[bin] with bin < 1024.
#include "common.hpp"
#include "kqv.hpp"
#include "kset.hpp"
#include "tiles.hpp"

namespace {

constexpr int KC_HIST_BLOCKS = 1024;   // kq_hist: at most this many workgroups stride over the slots

__device__ __forceinline__ uint32_t kc_ballot_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ void __launch_bounds__(KQ_THREADS) kq_count_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                             const int64_t *__restrict__ first, int n, int64_t n_runs, int k, uint64_t *tab, uint64_t slots,
                                                             uint32_t *cnt, unsigned long long *stat)
{
    const int64_t g = (int64_t)blockIdx.x * KQ_THREADS + threadIdx.x;
    const uint8_t *seq = bases;
    int64_t b0 = 0, b1 = 0;   // (a lane behind the last run owns nothing and reads nothing)
    if (g < n_runs) {
        const int c = kq_record_of(first, n, g);
        seq = bases + off[c];
        kq_deal(g - first[c], len[c], b0, b1);
    }
    KqRoll s = {0, 0, 0};
    if (b0 < b1) s = kq_lead(seq, b0, k);
    auto cas = [](uint64_t *p, uint64_t expect, uint64_t val) -> uint64_t {
        unsigned long long e = expect;
        (void)__hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long *>(p), &e, (unsigned long long)val, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        return (uint64_t)e;
    };
    auto stop = [stat]() -> bool { return __hip_atomic_load(stat + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; };
    auto load = [](uint32_t *p) -> uint32_t { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto add = [](uint32_t *p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    uint32_t n_pos = 0, n_new = 0;
    bool full = false;
    for (int r = 0; r < KQ_RUN; ++r) {   // (the same trip count in every lane: the ballots see the whole wave)
        int64_t pos;
        uint64_t key, at = 0;
        const bool has = kq_step(seq, b0, b1, r, s, k, pos, key);
        const int res = has ? kq_insert_at(tab, slots, key, cas, stop, at) : KQ_PRESENT;
        if (has && res != KQ_FULL) kq_bump(cnt + at, load, add);
        n_pos += kc_ballot_count(has && res != KQ_FULL);
        n_new += kc_ballot_count(res == KQ_NEW);
        full |= res == KQ_FULL;
    }
    if (full) (void)atomicOr(stat + 2, 1ull);
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) (void)atomicAdd(stat + 0, (unsigned long long)n_pos);
        if (n_new) (void)atomicAdd(stat + 1, (unsigned long long)n_new);
    }
}

__global__ void __launch_bounds__(256) kq_hist_kernel(const uint32_t *__restrict__ cnt, uint64_t slots, unsigned long long *hist)
{
    __shared__ uint32_t bins[KQ_BINS];
    for (int i = (int)threadIdx.x; i < KQ_BINS; i += 256) bins[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * 256) {
        const uint32_t c = cnt[i];
        if (c) (void)atomicAdd(&bins[kq_hist_bin(c)], 1u);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < KQ_BINS; i += 256)
        if (bins[i]) (void)atomicAdd(hist + i, (unsigned long long)bins[i]);
}

__global__ void __launch_bounds__(256) kq_seal_kernel(uint64_t *tab, const uint32_t *__restrict__ cnt, uint64_t slots, int channels, uint32_t m0, uint32_t m1,
                                                     unsigned long long *stat)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool s0 = false, s1 = false;
    if (i < slots) {
        const uint64_t key = tab[i];
        if (key != KQ_EMPTY) {
            s0 = kq_count_of(cnt[i]) >= m0;
            s1 = channels == 2 && kq_count_of(cnt[slots + i]) >= m1;
            tab[i] = kq_seal_word(key, channels, (s0 ? 1 : 0) | (s1 ? 2 : 0));
        }
    }
    const uint32_t n0 = kc_ballot_count(s0), n1 = kc_ballot_count(s1);   // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0) {
        if (n0) (void)atomicAdd(stat + 3, (unsigned long long)n0);
        if (n1) (void)atomicAdd(stat + 4, (unsigned long long)n1);
    }
}

// kq_copies: kq_insert's decomposition (a workgroup per tile of the set's tile table, a thread a run) with kq_count's walk: kq_insert_at() with the
// same stop poll and overflow word, then kq_copy_bump() on the slot's byte.  A key the reads never held is inserted here and keeps count 0; it is
// counted nowhere: stat[0] and stat[1] do not move, only the overflow word stat[2] can.
__global__ void __launch_bounds__(KQ_THREADS) kq_copies_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                              const int2 *__restrict__ tiles, int k, uint64_t *tab, uint64_t slots, uint32_t *cop,
                                                              unsigned long long *stat)
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
    auto load = [](uint32_t *p) -> uint32_t { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto cas32 = [](uint32_t *p, uint32_t expect, uint32_t val) -> uint32_t {
        uint32_t e = expect;
        (void)__hip_atomic_compare_exchange_strong(p, &e, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return e;
    };
    bool full = false;
    for (int r = 0; r < KQ_RUN; ++r) {
        int64_t pos;
        uint64_t key, at = 0;
        if (!kq_step(seq, b0, b1, r, s, k, pos, key)) continue;
        if (kq_insert_at(tab, slots, key, cas, stop, at) == KQ_FULL) full = true;
        else kq_copy_bump(cop + kq_copy_word(at), kq_copy_shift(at), load, cas32);
    }
    if (full) (void)atomicOr(stat + 2, 1ull);
}

// kq_spectrum: grid-stride over the slots as kq_hist, a workgroup's rounds in step so that the ballots see whole waves.  A slot with a count or a
// copy goes into its cell of 6 x 1024 uint32_t of LDS (a workgroup sees fewer than 2^32 slots); the non-zero cells are added with 64-bit atomics
// into the workspace the call zeroed.  out[KQ_CN_BINS * KQ_BINS] = solid, [.. + 1] = found, counted over the wave by ballots.  cop == nullptr: no
// copies call yet, every copy count reads 0.  Plain loads: complete at the kernel boundary.
__global__ void __launch_bounds__(256) kq_spectrum_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cop, uint64_t slots, uint32_t m,
                                                         unsigned long long *out)
{
    __shared__ uint32_t cells[KQ_CN_BINS * KQ_BINS];
    for (int i = (int)threadIdx.x; i < KQ_CN_BINS * KQ_BINS; i += 256) cells[i] = 0;
    __syncthreads();
    uint32_t n_solid = 0, n_found = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < slots; base += (uint64_t)gridDim.x * 256) {   // (the same trip count in every lane)
        const uint64_t i = base + threadIdx.x;
        uint32_t c = 0, a = 0;
        if (i < slots) {
            c = cnt[i];
            a = cop ? kq_copy_of(cop[kq_copy_word(i)], i) : 0;
        }
        if (c | a) (void)atomicAdd(&cells[kq_spec_cell(a, c)], 1u);
        const bool solid = c != 0 && kq_count_of(c) >= m;
        n_solid += kc_ballot_count(solid);
        n_found += kc_ballot_count(solid && a != 0);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < KQ_CN_BINS * KQ_BINS; i += 256)
        if (cells[i]) (void)atomicAdd(out + i, (unsigned long long)cells[i]);
    if ((threadIdx.x & 63) == 0) {
        if (n_solid) (void)atomicAdd(out + KQ_CN_BINS * KQ_BINS, (unsigned long long)n_solid);
        if (n_found) (void)atomicAdd(out + KQ_CN_BINS * KQ_BINS + 1, (unsigned long long)n_found);
    }
}

// kset_copies, kset_copies_clear, kset_spectrum: a counted set of one channel before its seal
int kc_copies_state(cornetto_accel_t *h, const cornetto_kset_t *s, const char *who)
{
    if (s->mode != KSET_COUNTED)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, s->counted ? "%s: the set is sealed; its counts are gone" : "%s: the set is not a counted one (kset_open_counted)", who);
    if (s->channels != 1) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "%s: copies go with a counted set of one channel; this one has %d", who, (int)s->channels);
    return CORNETTO_OK;
}

}  // namespace

extern "C" {

int cornetto_kset_copies(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a)
{
    if (!h || !s || !a) return cn_fail(h, CORNETTO_E_ARG, "kset_copies: bad argument");
    CN_TRY(kc_copies_state(h, s, "kset_copies"));
    if (s->dead) return cn_fail(h, CORNETTO_E_NOMEM, "kset_copies: the table of %lld slots has overflowed; the set is unusable", (long long)s->slots);
    CN_HIP(h, hipSetDevice(h->device));
    if (!s->d_cop) {   // allocated at the first call, not at the open: a set that never sees an assembly stays at 12 bytes a slot
        const size_t bytes = (size_t)kq_copy_words((uint64_t)s->slots) * 4;
        if (hipMalloc((void **)&s->d_cop, bytes) != hipSuccess) {
            (void)hipGetLastError();
            s->d_cop = nullptr;
            return cn_fail(h, CORNETTO_E_NOMEM, "kset_copies: the copy counts of %lld slots wanted %lld bytes of device memory", (long long)s->slots, (long long)bytes);
        }
        if (hipMemsetAsync(s->d_cop, 0, bytes, h->stream) != hipSuccess) {   // every byte 0, whatever the memory held
            (void)hipFree(s->d_cop);
            s->d_cop = nullptr;
            return cn_fail(h, CORNETTO_E_HIP, "kset_copies: the copy counts could not be cleared");
        }
    }
    cn_timing_begin(h);
    const int64_t nt = kq_tiles(h, s, a);
    if (nt < 0) return (int)nt;
    unsigned long long *p_stat = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!p_stat) return cn_fail(h, CORNETTO_E_NOMEM, "kset_copies: host allocation failed");
    if (nt > 0)
        CN_LAUNCH(h, "kq_copies", kq_copies_kernel<<<dim3((unsigned)nt), dim3(KQ_THREADS), 0, h->stream>>>(a->d_bases, a->d_off, a->d_len, s->d_tiles, s->k, s->d_tab,
                                                                                                          (uint64_t)s->slots, s->d_cop, s->d_stat));
    if (nt > 0) s->copied = true;   // from here on the table may hold assembly-only keys; a call that failed in front of its launch has touched nothing
    CN_HIP(h, hipMemcpyAsync(p_stat, s->d_stat, 24, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    if (p_stat[2]) {
        s->dead = true;
        return cn_fail(h, CORNETTO_E_NOMEM, "kset_copies: the table of %lld slots overflowed (the assembly holds k-mers the reads do not, and each takes a slot); the set is unusable",
                       (long long)s->slots);
    }
    return CORNETTO_OK;
}

int cornetto_kset_copies_clear(cornetto_accel_t *h, cornetto_kset_t *s)
{
    if (!h || !s) return cn_fail(h, CORNETTO_E_ARG, "kset_copies_clear: bad argument");
    CN_TRY(kc_copies_state(h, s, "kset_copies_clear"));
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_copies_clear: the set is unusable, its table has overflowed");
    if (!s->d_cop) return CORNETTO_OK;
    CN_HIP(h, hipSetDevice(h->device));
    CN_HIP(h, hipMemsetAsync(s->d_cop, 0, (size_t)kq_copy_words((uint64_t)s->slots) * 4, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    return CORNETTO_OK;
}

int cornetto_kset_spectrum(cornetto_accel_t *h, cornetto_kset_t *s, int32_t channel, int32_t min_count, int64_t *spec, int64_t *totals)
{
    if (!h || !s || !spec || !totals) return cn_fail(h, CORNETTO_E_ARG, "kset_spectrum: bad argument");
    CN_TRY(kc_copies_state(h, s, "kset_spectrum"));
    if (channel != 0) return cn_fail(h, CORNETTO_E_ARG, "kset_spectrum: channel %d of a set of %d", (int)channel, (int)s->channels);
    if (min_count < 1 || min_count > CORNETTO_KSET_COUNT_CAP)
        return cn_fail(h, CORNETTO_E_ARG, "kset_spectrum: min_count = %d; a threshold is 1 to %d", (int)min_count, CORNETTO_KSET_COUNT_CAP);
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_spectrum: the set is unusable, its table has overflowed");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    constexpr size_t N = (size_t)KQ_CN_BINS * KQ_BINS + 2;
    unsigned long long *d_out = (unsigned long long *)cn_ws(h, WS_KC_HIST, N * 8);
    unsigned long long *p_out = (unsigned long long *)cn_pin(h, PIN_SMALL, N * 8);
    if (!d_out || !p_out) return cn_fail(h, CORNETTO_E_NOMEM, "kset_spectrum: workspace allocation failed");
    CN_HIP(h, hipMemsetAsync(d_out, 0, N * 8, h->stream));
    const int64_t want = (s->slots + 255) / 256;
    const unsigned nb = (unsigned)(want < KC_HIST_BLOCKS ? want : KC_HIST_BLOCKS);
    CN_LAUNCH(h, "kq_spectrum", kq_spectrum_kernel<<<dim3(nb), dim3(256), 0, h->stream>>>(s->d_cnt, s->d_cop, (uint64_t)s->slots, (uint32_t)min_count, d_out));
    CN_HIP(h, hipMemcpyAsync(p_out, d_out, N * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    for (size_t i = 0; i < N - 2; ++i) spec[i] = (int64_t)p_out[i];
    totals[0] = (int64_t)p_out[N - 2];
    totals[1] = (int64_t)p_out[N - 1];
    return CORNETTO_OK;
}

int cornetto_kset_open_counted(cornetto_accel_t *h, int32_t k, int64_t slots, int32_t channels, cornetto_kset_t **out)
{
    if (channels != 1 && channels != 2) {
        if (out) *out = nullptr;
        return cn_fail(h, CORNETTO_E_ARG, "kset_open_counted: bad argument (a counted set has 1 or 2 channels)");
    }
    return kq_open(h, "kset_open_counted", k, slots, channels, out);
}

int cornetto_kset_count(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a, int32_t channel)
{
    if (!h || !s || !a) return cn_fail(h, CORNETTO_E_ARG, "kset_count: bad argument");
    if (s->mode != KSET_COUNTED)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, s->counted ? "kset_count: the set is sealed; it takes no more counts" : "kset_count: the set is not a counted one (kset_open_counted)");
    if (s->copied) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_count: the set has seen kset_copies; it may hold keys of an assembly and takes no more counts");
    if (channel < 0 || channel >= s->channels) return cn_fail(h, CORNETTO_E_ARG, "kset_count: channel %d of a set of %d", (int)channel, (int)s->channels);
    if (s->dead) return cn_fail(h, CORNETTO_E_NOMEM, "kset_count: the table of %lld slots has overflowed; the set is unusable", (long long)s->slots);
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    const int64_t nr = cntiles::prefix(h, s->pref, a->n, [&](int32_t c) { return kq_runs_of((int64_t)a->len[c]); });
    if (nr < 0) return cn_fail(h, CORNETTO_E_NOMEM, "kset_count: device allocation failed");
    const int64_t nb = (nr + KQ_THREADS - 1) / KQ_THREADS;
    if (nb > 0x7fffffffll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_count: too many runs in one batch");
    unsigned long long *p_stat = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!p_stat) return cn_fail(h, CORNETTO_E_NOMEM, "kset_count: host allocation failed");
    if (nb > 0)
        CN_LAUNCH(h, "kq_count", kq_count_kernel<<<dim3((unsigned)nb), dim3(KQ_THREADS), 0, h->stream>>>(a->d_bases, a->d_off, a->d_len, s->pref.dev, a->n, nr, s->k, s->d_tab,
                                                                                                        (uint64_t)s->slots, s->d_cnt + (size_t)channel * (size_t)s->slots,
                                                                                                        s->d_stat));
    CN_HIP(h, hipMemcpyAsync(p_stat, s->d_stat, 24, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    s->stats[0] = (int64_t)p_stat[0];
    s->stats[1] = (int64_t)p_stat[1];
    if (p_stat[2]) {
        s->dead = true;
        return cn_fail(h, CORNETTO_E_NOMEM, "kset_count: the table of %lld slots overflowed (%lld distinct k-mers are in it); the set is unusable", (long long)s->slots,
                       (long long)s->stats[1]);
    }
    return CORNETTO_OK;
}

int cornetto_kset_hist(cornetto_accel_t *h, cornetto_kset_t *s, int32_t channel, int64_t *hist)
{
    if (!h || !s || !hist) return cn_fail(h, CORNETTO_E_ARG, "kset_hist: bad argument");
    if (s->mode != KSET_COUNTED)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, s->counted ? "kset_hist: the set is sealed; its counts are gone" : "kset_hist: the set is not a counted one (kset_open_counted)");
    if (channel < 0 || channel >= s->channels) return cn_fail(h, CORNETTO_E_ARG, "kset_hist: channel %d of a set of %d", (int)channel, (int)s->channels);
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_hist: the set is unusable, its table has overflowed");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    unsigned long long *d_hist = (unsigned long long *)cn_ws(h, WS_KC_HIST, KQ_BINS * 8);
    unsigned long long *p_hist = (unsigned long long *)cn_pin(h, PIN_SMALL, KQ_BINS * 8);
    if (!d_hist || !p_hist) return cn_fail(h, CORNETTO_E_NOMEM, "kset_hist: workspace allocation failed");
    CN_HIP(h, hipMemsetAsync(d_hist, 0, KQ_BINS * 8, h->stream));
    const int64_t want = (s->slots + 255) / 256;
    const unsigned nb = (unsigned)(want < KC_HIST_BLOCKS ? want : KC_HIST_BLOCKS);
    CN_LAUNCH(h, "kq_hist", kq_hist_kernel<<<dim3(nb), dim3(256), 0, h->stream>>>(s->d_cnt + (size_t)channel * (size_t)s->slots, (uint64_t)s->slots, d_hist));
    CN_HIP(h, hipMemcpyAsync(p_hist, d_hist, KQ_BINS * 8, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    for (int i = 0; i < KQ_BINS; ++i) hist[i] = (int64_t)p_hist[i];
    return CORNETTO_OK;
}

int cornetto_kset_seal(cornetto_accel_t *h, cornetto_kset_t *s, const int32_t *min_count, int64_t *solid)
{
    if (!h || !s || !min_count || !solid) return cn_fail(h, CORNETTO_E_ARG, "kset_seal: bad argument");
    if (s->mode != KSET_COUNTED)
        return cn_fail(h, CORNETTO_E_UNSUPPORTED, s->counted ? "kset_seal: the set is sealed already" : "kset_seal: the set is not a counted one (kset_open_counted)");
    for (int c = 0; c < s->channels; ++c)
        if (min_count[c] < 1 || min_count[c] > CORNETTO_KSET_COUNT_CAP)
            return cn_fail(h, CORNETTO_E_ARG, "kset_seal: min_count[%d] = %d; a threshold is 1 to %d", c, (int)min_count[c], CORNETTO_KSET_COUNT_CAP);
    if (s->dead) return cn_fail(h, CORNETTO_E_ARG, "kset_seal: the set is unusable, its table has overflowed");
    CN_HIP(h, hipSetDevice(h->device));
    cn_timing_begin(h);
    unsigned long long *p_stat = (unsigned long long *)cn_pin(h, PIN_SMALL, 64);
    if (!p_stat) return cn_fail(h, CORNETTO_E_NOMEM, "kset_seal: host allocation failed");
    const int64_t nb = (s->slots + 255) / 256;
    if (nb > 0x7fffffffll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset_seal: too many slots");
    CN_HIP(h, hipMemsetAsync(s->d_stat + 3, 0, 16, h->stream));
    CN_LAUNCH(h, "kq_seal", kq_seal_kernel<<<dim3((unsigned)nb), dim3(256), 0, h->stream>>>(s->d_tab, s->d_cnt, (uint64_t)s->slots, (int)s->channels, (uint32_t)min_count[0],
                                                                                           (uint32_t)(s->channels == 2 ? min_count[1] : 1), s->d_stat));
    CN_HIP(h, hipMemcpyAsync(p_stat, s->d_stat + 3, 16, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    cn_timing_end(h);
    for (int c = 0; c < s->channels; ++c) solid[c] = (int64_t)p_stat[c];
    (void)hipFree(s->d_cnt);
    s->d_cnt = nullptr;
    if (s->d_cop) (void)hipFree(s->d_cop);
    s->d_cop = nullptr;
    s->mode = s->channels == 1 ? KSET_PLAIN : KSET_TAGGED;
    return CORNETTO_OK;
}

}  // extern "C"
