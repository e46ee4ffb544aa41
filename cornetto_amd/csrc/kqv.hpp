// kqv.hpp — the arithmetic of `cornetto qv` (include/cornetto_accel.h states the rule): canonical k-mers of a contig by a rolling update, an
// open-addressing set of them, and the bitmap of the positions a query misses.  Shared by the kernels of kqv.hip and, as a CPU program under the
// host sanitizers, by tools/sim/kqv_sim.cc (tests/test_kqv_host.py), so everything here is a host/device function over plain pointers.
//   kq_code()     a byte's base code 0..3, or 4 for every other byte;
//   kq_roll()     one base into {fwd, rc, valid}: fwd and rc are the 2k-bit codes of the last k bases and of their reverse complement (first
//                 base most significant), valid counts the valid bases behind the position, capped at k; an invalid byte sets it to 0;
//   kq_run()      the decomposition: a contig is cut into tiles of KQ_TILE bases, thread `tid` of a tile owns the KQ_RUN consecutive bases
//                 [b0, b1) and with them the k-mers that END there (position e - k + 1 for base e).  It rolls the k - 1 bases in front of b0
//                 in first — the first run of a contig has nothing in front — and calls f(position, canonical k-mer) for every owned base
//                 with valid == k.  It reads seq[max(b0 - k + 1, 0) .. b1), b1 <= len: never a byte outside the contig;
//   kq_home()     the home slot mulhi64(mix(key), slots): slots need not be a power of two;
//   kq_insert()   linear probing from the home slot through cas(slot, EMPTY, key) -> the old value: done when that is EMPTY (new) or the key
//                 itself; at most `slots` steps, then KQ_FULL.  `stop()` lets the lanes of a kernel leave once one of them has overflowed;
//   kq_lookup()   the same walk with plain loads; a key is missing at the first EMPTY slot or after `slots` steps;
//   kq_bit()      word and mask of position `pos` of a contig whose first tile is `tile0` in the bitmap (KQ_TILE bits per tile).
//   kq_insert_tag(), kq_lookup_tag()   the same table with a 2-bit tag in bits 63:62 of a slot, for `cornetto trioeval` (ktrio.hip): below.
//   kq_deal(), kq_insert_at(), kq_bump(), kq_hist_bin(), kq_seal_word()   the counted table of `qv -r` / `trioeval --pat-reads` (kcount.hip): at the end.
//   kq_copy_bump(), kq_copy_word(), kq_copy_shift(), kq_copy_of(), kq_spec_cell()   the copies of `qv -r --completeness / --spectra-cn`: behind them.
// The empty slot is ~0: no key, k <= 31 makes every key smaller than 2^62.
#pragma once
#include <cstdint>

#include "../../include/cornetto_accel.h"

#ifdef __HIPCC__
#define KQ_HD __host__ __device__
#else
#define KQ_HD
#endif

namespace {   // internal linkage: every translation unit that includes this gets its own copy

constexpr int KQ_THREADS = 256;                        // threads per workgroup = per tile
constexpr int KQ_RUN = CORNETTO_KQV_TILE / KQ_THREADS; // consecutive bases per thread
constexpr int KQ_TILE = CORNETTO_KQV_TILE;
static_assert(KQ_RUN * KQ_THREADS == KQ_TILE && KQ_TILE % 64 == 0, "a tile is whole runs and whole bitmap words");
constexpr uint64_t KQ_EMPTY = ~(uint64_t)0;
constexpr int KQ_NEW = 1, KQ_PRESENT = 0, KQ_FULL = -1;

KQ_HD static inline bool kq_k_ok(int k) { return k >= 11 && k <= 31 && (k & 1); }

KQ_HD static inline int kq_code(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

struct KqRoll {
    uint64_t fwd, rc;
    int valid;
};

KQ_HD static inline void kq_roll(KqRoll &s, int code, int k)
{
    if (code > 3) {
        s.valid = 0;
        return;
    }
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    s.fwd = ((s.fwd << 2) | (uint64_t)code) & mask;
    s.rc = (s.rc >> 2) | ((uint64_t)(3 - code) << (2 * (k - 1)));
    if (s.valid < k) ++s.valid;
}

KQ_HD static inline uint64_t kq_canon(const KqRoll &s) { return s.fwd < s.rc ? s.fwd : s.rc; }

// the owned bases [b0, b1) of thread `tid` of the tile that begins at base `first` of a contig of `len` bases (b0 >= b1: none)
KQ_HD static inline void kq_bounds(int64_t first, int tid, int64_t len, int64_t &b0, int64_t &b1)
{
    b0 = first + (int64_t)tid * KQ_RUN;
    b1 = b0 + KQ_RUN < len ? b0 + KQ_RUN : len;
}

// the state in front of base b0: the up to k - 1 bases before it rolled in
KQ_HD static inline KqRoll kq_lead(const uint8_t *seq, int64_t b0, int k)
{
    KqRoll s = {0, 0, 0};
    for (int64_t i = b0 - (k - 1) > 0 ? b0 - (k - 1) : 0; i < b0; ++i) kq_roll(s, kq_code(seq[i]), k);
    return s;
}

// base b0 + r of the run [b0, b1) rolled into s; true when a k-mer ends there: its position and its canonical code.  r >= b1 - b0: nothing is read
KQ_HD static inline bool kq_step(const uint8_t *seq, int64_t b0, int64_t b1, int r, KqRoll &s, int k, int64_t &pos, uint64_t &key)
{
    const int64_t e = b0 + r;
    if (e >= b1) return false;
    kq_roll(s, kq_code(seq[e]), k);
    if (s.valid != k) return false;
    pos = e - (k - 1);
    key = kq_canon(s);
    return true;
}

// a thread of the kernels: bounds, lead, KQ_RUN steps (the kernels spell the same three calls out, with their ballots between the steps)
template <class F>
KQ_HD static inline void kq_run(const uint8_t *seq, int64_t len, int64_t first, int tid, int k, F f)
{
    int64_t b0, b1;
    kq_bounds(first, tid, len, b0, b1);
    KqRoll s = {0, 0, 0};
    if (b0 < b1) s = kq_lead(seq, b0, k);
    for (int r = 0; r < KQ_RUN; ++r) {
        int64_t pos;
        uint64_t key;
        if (kq_step(seq, b0, b1, r, s, k, pos, key)) f(pos, key);
    }
}

// the finaliser of MurmurHash3 (public domain): every input bit reaches every output bit
KQ_HD static inline uint64_t kq_mix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

KQ_HD static inline uint64_t kq_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

KQ_HD static inline uint64_t kq_home(uint64_t key, uint64_t slots) { return kq_mulhi(kq_mix(key), slots); }   // < slots
KQ_HD static inline uint64_t kq_next(uint64_t slot, uint64_t slots) { return slot + 1 == slots ? 0 : slot + 1; }

// the walk of kq_insert(); `at` = the slot the key sits in (untouched on KQ_FULL), which the counted table of kcount.hip adds its count at
template <class Cas, class Stop>
KQ_HD static inline int kq_insert_at(uint64_t *tab, uint64_t slots, uint64_t key, Cas cas, Stop stop, uint64_t &at)
{
    uint64_t slot = kq_home(key, slots);
    for (uint64_t step = 0; step < slots; ++step) {
        const uint64_t old = cas(tab + slot, KQ_EMPTY, key);
        if (old == KQ_EMPTY || old == key) {
            at = slot;
            return old == key ? KQ_PRESENT : KQ_NEW;
        }
        if ((step & 1023) == 1023 && stop()) return KQ_FULL;
        slot = kq_next(slot, slots);
    }
    return KQ_FULL;
}

template <class Cas, class Stop>
KQ_HD static inline int kq_insert(uint64_t *tab, uint64_t slots, uint64_t key, Cas cas, Stop stop)
{
    uint64_t at;
    return kq_insert_at(tab, slots, key, cas, stop, at);
}

KQ_HD static inline bool kq_lookup(const uint64_t *tab, uint64_t slots, uint64_t key)
{
    uint64_t slot = kq_home(key, slots);
    for (uint64_t step = 0; step < slots; ++step) {
        const uint64_t v = tab[slot];
        if (v == key) return true;
        if (v == KQ_EMPTY) return false;
        slot = kq_next(slot, slots);
    }
    return false;
}

// ---- the tagged table of `cornetto trioeval`: a slot holds key | tag << 62, tag bit 0 = the key came from a paternal input, bit 1 = from a
// maternal one; a table is either plain or tagged (cornetto_kset keeps which).  The empty slot stays ~0, and no tagged slot equals it: that
// would take tag 3 and the key 2^62 - 1.  For k < 31 a key is below 2^(2k) <= 2^58.  For k = 31 the all-ones 62-bit code is T...T, whose
// reverse complement A...A is 0 — the canonical code of that k-mer is 0, so 2^62 - 1 is never a key.
//   kq_insert_tag()   old = cas(slot, EMPTY, key | tag << 62): new when old is EMPTY; when old holds the key under KQ_KEYMASK, the tag is OR-ed in
//                     with fetch_or(slot, tag << 62) -> the old value — skipped when `old` carries it already (tags are only ever added, so a
//                     value an atomic returned never overstates them) — and the key is present; otherwise the next slot.  The same `slots`-step
//                     bound, KQ_FULL and stop() poll as kq_insert(); as there, only values returned by atomics decide anything;
//   kq_lookup_tag()   plain loads (complete at the kernel boundary), compare under KQ_KEYMASK -> the tag, 0 for an absent key.
constexpr uint64_t KQ_KEYMASK = ((uint64_t)1 << 62) - 1;
constexpr int KQ_TAG_SHIFT = 62;

template <class Cas, class FetchOr, class Stop>
KQ_HD static inline int kq_insert_tag(uint64_t *tab, uint64_t slots, uint64_t key, uint64_t tag, Cas cas, FetchOr fetch_or, Stop stop)
{
    const uint64_t bits = tag << KQ_TAG_SHIFT;
    uint64_t slot = kq_home(key, slots);
    for (uint64_t step = 0; step < slots; ++step) {
        const uint64_t old = cas(tab + slot, KQ_EMPTY, key | bits);
        if (old == KQ_EMPTY) return KQ_NEW;
        if ((old & KQ_KEYMASK) == key) {
            if ((old & bits) != bits) (void)fetch_or(tab + slot, bits);
            return KQ_PRESENT;
        }
        if ((step & 1023) == 1023 && stop()) return KQ_FULL;
        slot = kq_next(slot, slots);
    }
    return KQ_FULL;
}

KQ_HD static inline int kq_lookup_tag(const uint64_t *tab, uint64_t slots, uint64_t key)
{
    uint64_t slot = kq_home(key, slots);
    for (uint64_t step = 0; step < slots; ++step) {
        const uint64_t v = tab[slot];
        if (v == KQ_EMPTY) return 0;
        if ((v & KQ_KEYMASK) == key) return (int)(v >> KQ_TAG_SHIFT);
        slot = kq_next(slot, slots);
    }
    return 0;
}

// position `pos` of a contig whose first tile is tile `tile0` of the table: bit `pos` behind the contig's first word
KQ_HD static inline void kq_bit(int64_t tile0, int64_t pos, int64_t &word, uint64_t &mask)
{
    const int64_t g = tile0 * KQ_TILE + pos;
    word = g >> 6;
    mask = (uint64_t)1 << (g & 63);
}

// ---- the bitmap -> the runs of consecutive set bits.  Word w with the last bit of the word in front (`prev`, 0 for the first word) and the
// first bit of the word behind (`next`, 0 for the last): a run starts at a set bit whose predecessor is clear and ends at a set bit whose
// successor is clear.  No run spans two contigs: the last k - 1 positions of a contig hold no k-mer, so the bit in front of a contig's first
// word is always clear.  The j-th start of the bitmap and its j-th end are the same run; with rank = starts in front of word w, the ends
// in front of it are rank - (a run is open across the seam: prev && the word's first bit).
KQ_HD static inline uint64_t kq_starts(uint64_t w, uint64_t prev) { return w & ~((w << 1) | (prev & 1)); }
KQ_HD static inline uint64_t kq_ends(uint64_t w, uint64_t next) { return w & ~((w >> 1) | ((next & 1) << 63)); }
KQ_HD static inline uint32_t kq_end_rank(uint32_t rank, uint64_t w, uint64_t prev) { return rank - (uint32_t)(prev & w & 1); }

// ---- the counted table of `cornetto qv -r` and `cornetto trioeval --pat-reads / --mat-reads` (kcount.hip; include/cornetto_accel.h states the
// rule).  The table of keys is the plain one above; beside it stand channels * slots uint32_t counts, count[ch * slots + slot] for the key in
// `slot`.  Sealing with thresholds turns the table into the plain or the tagged one in place, so kq_lookup() / kq_lookup_tag() and the kernels
// around them serve a sealed set unchanged.
//   kq_deal()       the decomposition of a batch of (short) records: lanes are dealt runs, not records.  first[c] = sum over the records in front
//                   of c of ceil(len / KQ_RUN); run g of the batch is run g - first[c] of its record c = kq_record_of(), the bases [b0, b1) of it, with
//                   b1 <= len: kq_lead() + kq_step() on them read seq[max(b0 - k + 1, 0) .. b1), never a byte outside the record;
//   kq_bump()       one occurrence into a count that must never wrap: the add is issued only while a load of the count reads below
//                   CORNETTO_KSET_COUNT_CAP.  Counts only grow, so (1) while fewer than CAP occurrences have been added every load reads below CAP
//                   and no add is skipped: a true count below CAP is stored exactly; (2) if the stored value ended below CAP, every load would
//                   have read below CAP and every add would have been issued, so a true count of CAP or more ends at CAP or more.  Hence
//                   min(stored, CAP) = min(true, CAP), whatever the order.  (3) An add is issued only by a lane whose load read below CAP; after the
//                   value reaches CAP only the lanes that loaded before that still add, so stored < CAP + lanes in flight on the device
//                   (< 2^20 on 256 CUs of 2048 lanes) — far from 2^32, also across launches, since every launch starts from a stored value
//                   that obeys the same bound and a value of CAP or more admits no new add;
//   kq_count_of()   min(stored, CAP): the count of the rule;
//   kq_hist_bin()   min(count, BINS - 1): the histogram bin of a key, 0 for a key this channel never saw;
//   kq_seal_word()  the slot's word after sealing: `tag` = bit ch set iff the key is solid in channel ch.  One channel: the key, or KQ_TOMB.  Two:
//                   key | tag << 62, or KQ_TOMB for tag 0.
// KQ_TOMB = KQ_EMPTY - 1 = 2^64 - 2 marks an occupied slot whose key is solid nowhere: a walk passes it (only KQ_EMPTY ends a walk, so keys behind
// a removed one stay reachable) and no key matches it.  kq_lookup() compares the whole word, and every key is below 2^62.  kq_lookup_tag() compares
// under KQ_KEYMASK, where the tombstone reads 2^62 - 2: for k < 31 every key is below 2^58; for k = 31 the code 2^62 - 2 is T...TG, whose reverse
// complement CA...A = 2^60 is smaller, so the canonical code of that k-mer is 2^60 and 2^62 - 2 is never a key.  No sealed word equals KQ_EMPTY
// (kq_insert_tag's argument above) and none but the tombstone equals KQ_TOMB: that would take tag 3 and the key 2^62 - 2.
constexpr uint64_t KQ_TOMB = KQ_EMPTY - 1;
constexpr uint32_t KQ_CAP = CORNETTO_KSET_COUNT_CAP;
constexpr int KQ_BINS = CORNETTO_KSET_HIST_BINS;
static_assert((uint32_t)(KQ_BINS - 1) <= KQ_CAP, "the last bin lies at or below the cap: min(stored, BINS - 1) is the bin of min(stored, CAP)");

KQ_HD static inline int64_t kq_runs_of(int64_t len) { return (len + KQ_RUN - 1) / KQ_RUN; }

// the record c with first[c] <= g < first[c + 1] (first[0] = 0 <= g < first[n]; records without a run are skipped): tiles.hpp's bisection
KQ_HD static inline int kq_record_of(const int64_t *first, int n, int64_t g)
{
    int lo = 0, hi = n;   // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// run j of a record of `len` bases -> its bases [b0, b1)
KQ_HD static inline void kq_deal(int64_t j, int64_t len, int64_t &b0, int64_t &b1)
{
    b0 = j * KQ_RUN;
    b1 = b0 + KQ_RUN < len ? b0 + KQ_RUN : len;
}

template <class Load, class Add>
KQ_HD static inline void kq_bump(uint32_t *c, Load load, Add add)
{
    if (load(c) < KQ_CAP) add(c);
}

KQ_HD static inline uint32_t kq_count_of(uint32_t stored) { return stored < KQ_CAP ? stored : KQ_CAP; }
KQ_HD static inline int kq_hist_bin(uint32_t stored) { return stored < (uint32_t)(KQ_BINS - 1) ? (int)stored : KQ_BINS - 1; }

KQ_HD static inline uint64_t kq_seal_word(uint64_t key, int channels, int tag)
{
    if (!tag) return KQ_TOMB;
    return channels == 1 ? key : key | (uint64_t)tag << KQ_TAG_SHIFT;
}

// ---- the copies of `cornetto qv -r --completeness / --spectra-cn` (kcount.hip: kq_copies, kq_spectrum; include/cornetto_accel.h states the rule).
// Beside the counts of a one-channel counted table stands one BYTE per slot, copies[slot] = min(occurrences of the slot's key in the assembly,
// KQ_CN_MAX), packed four to a uint32_t: slot i is byte i & 3 (bits 8 * (i & 3) ..) of word i >> 2, ceil(slots / 4) words.
//   kq_copy_bump()   one occurrence into the byte at `shift` of `word`: a relaxed load of the word; leave if the byte reads KQ_CN_MAX (or more: it
//                    never does); else cas(word, seen, seen + (1 << shift)) -> the word that was there; done when that is `seen`, else it becomes
//                    `seen` and the step repeats.  Termination and exactness: the bytes only grow between two clears.  A compare-and-swap fails
//                    only when the word differs from `seen`, i.e. when another lane's compare-and-swap on that word has succeeded since `seen`
//                    was read.  A success raises one byte by one and happens only on a word whose byte was seen below KQ_CN_MAX IN THAT SAME WORD
//                    VALUE — the swap stores seen + 1 in the byte only if the word still is `seen` — so a byte takes at most KQ_CN_MAX = 5
//                    successes between two clears and a word at most 20: no lane fails more than 19 times.  Every occurrence either succeeds
//                    once or leaves at a byte that reads 5, and a byte below 5 turns no occurrence away, so the stored byte is exactly
//                    min(occurrences, 5).  There is no overshoot to bound, unlike kq_bump(): an add of 1 << shift behind a load check could pass 5
//                    by the lanes in flight and carry into the neighbour's byte;
//   kq_spec_cell()   the cell of a key in the 6 x 1024 spectrum: min(copies, 5) * KQ_BINS + kq_hist_bin(stored count).  A slot with count 0 and
//                    copies 0 — empty, or an assembly-only key after a clear — is in no cell: the kernels skip it.
constexpr int KQ_CN_BINS = CORNETTO_KSET_CN_BINS;
constexpr uint32_t KQ_CN_MAX = KQ_CN_BINS - 1;
static_assert(KQ_CN_MAX < 255, "a copy count is a byte");

KQ_HD static inline uint64_t kq_copy_words(uint64_t slots) { return (slots + 3) >> 2; }
KQ_HD static inline uint64_t kq_copy_word(uint64_t slot) { return slot >> 2; }   // < kq_copy_words(slots) for slot < slots
KQ_HD static inline int kq_copy_shift(uint64_t slot) { return (int)(slot & 3) * 8; }
KQ_HD static inline uint32_t kq_copy_of(uint32_t word, uint64_t slot) { return (word >> kq_copy_shift(slot)) & 0xFFu; }

template <class Load, class Cas>
KQ_HD static inline void kq_copy_bump(uint32_t *word, int shift, Load load, Cas cas)
{
    uint32_t seen = load(word);
    while (((seen >> shift) & 0xFFu) < KQ_CN_MAX) {
        const uint32_t old = cas(word, seen, seen + ((uint32_t)1 << shift));
        if (old == seen) return;
        seen = old;
    }
}

KQ_HD static inline int kq_spec_cell(uint32_t copies, uint32_t stored)
{
    return (int)(copies < KQ_CN_MAX ? copies : KQ_CN_MAX) * KQ_BINS + kq_hist_bin(stored);
}

}  // namespace
