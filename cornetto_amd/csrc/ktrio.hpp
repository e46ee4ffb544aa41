// ktrio.hpp — the ordered pass of `cornetto trioeval` (include/cornetto_accel.h states the rule): from the two bitmaps of marked positions (pat,
// mat; disjoint; KQ_TILE bits per tile, kq_bit() of kqv.hpp) to the pair counts pp, pm, mp, mm of every contig — each marker with the type of the
// nearest marker in front of it in the same contig.  Shared by the kernels of ktrio.hip and, as a CPU program under the host sanitizers, by
// tools/sim/ktrio_sim.cc (tests/test_ktrio_host.py), so everything here is a host/device function over plain values and pointers.
// Types: KT_NONE 0, KT_PAT 1, KT_MAT 2 (a tag of the table with exactly one bit).  A pair (prev, own) has the index kt_pair(): pp 0, pm 1, mp 2, mm 3.
//   the word  kt_word(): a lane holds word p of the pat bitmap and word m of the mat bitmap.  g = the positions whose last marker AT OR BELOW them
//             in the word is pat: a prefix fill of p's bits upwards through marker-free positions, stopped by a bit of m (6 doubling steps, the
//             carry chain of an adder with generate p and propagate ~(p | m)); gm the same for mat = (at or above the word's first marker) & ~g.
//             A marker at bit i > first pairs with the type at bit i - 1: popcounts of p and m against g << 1 and gm << 1.  The word's first
//             marker pairs with `in`, the type of the last marker in front of the word (none: no pair);
//   the wave  a tile is KT_WORDS = 64 words, lane l = word l.  `in` of lane l is the exclusive scan of kt_last() over the lanes with kt_op(a, b) =
//             b unless b is none — "the right operand unless it is none" is associative: (a op b) op c and a op (b op c) are both the last
//             operand that is not none — so the 6 shuffle steps of a wave scan give it.  In front of lane 0 stands none: the pair across the
//             tile's front seam is kt_seam's.  A tile leaves one byte, kt_tile_byte(first, last): the types of its first and last marker;
//   the seam  a tile with a marker that is not its contig's first tile looks back for the nearest tile with last != none, KT_WORDS tiles a round,
//             lane l of a round at tile hi - 1 - l, never in front of the contig's first tile t0 (kt_seam_look()); the nearest is the lowest
//             lane that found one.  The one pair (that last, own first) is added; no tile found: the tile holds the contig's first marker.
#pragma once
#include "kqv.hpp"

namespace {

constexpr int KT_NONE = 0, KT_PAT = 1, KT_MAT = 2;
constexpr int KT_WORDS = KQ_TILE / 64;     // words of a tile's bitmap = lanes of the wave that owns it
static_assert(KT_WORDS == 64, "kt_tile gives a lane a word and a wave a tile");
constexpr int KT_COUNTS = CORNETTO_TRIO_COUNTS;   // per contig: kmers, pat, mat, pp, pm, mp, mm

KQ_HD static inline int kt_pair(int prev, int own) { return (prev - 1) * 2 + (own - 1); }
KQ_HD static inline int kt_op(int a, int b) { return b != KT_NONE ? b : a; }
KQ_HD static inline int kt_popc(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll((unsigned long long)x);
#else
    return __builtin_popcountll(x);
#endif
}

// the type of the word's first (lowest) and last (highest) marker; p & m == 0
KQ_HD static inline int kt_first(uint64_t p, uint64_t m)
{
    const uint64_t a = p | m;
    if (!a) return KT_NONE;
    return (a & (~a + 1)) & p ? KT_PAT : KT_MAT;
}
KQ_HD static inline int kt_last(uint64_t p, uint64_t m) { return !(p | m) ? KT_NONE : p > m ? KT_PAT : KT_MAT; }   // disjoint: the larger word holds the highest bit

// the positions of the word whose last marker at or below them is a bit of p
KQ_HD static inline uint64_t kt_fill(uint64_t p, uint64_t m)
{
    uint64_t g = p, pr = ~(p | m);
    for (int d = 1; d < 64; d <<= 1) {
        g |= pr & (g << d);
        pr &= pr << d;
    }
    return g;
}

// the pairs of the word's markers, packed 16 bits a count (pp, pm, mp, mm from the low end; a tile has at most KQ_TILE < 2^16 pairs)
KQ_HD static inline uint64_t kt_word(uint64_t p, uint64_t m, int in)
{
    const uint64_t a = p | m;
    if (!a) return 0;
    const uint64_t low = a & (~a + 1);
    const uint64_t g = kt_fill(p, m), gm = ~(low - 1) & ~g;
    const uint64_t prev_p = g << 1, prev_m = gm << 1;
    uint64_t r = (uint64_t)kt_popc(p & prev_p) | (uint64_t)kt_popc(m & prev_p) << 16 | (uint64_t)kt_popc(p & prev_m) << 32 | (uint64_t)kt_popc(m & prev_m) << 48;
    if (in != KT_NONE) r += (uint64_t)1 << (16 * kt_pair(in, low & p ? KT_PAT : KT_MAT));
    return r;
}

KQ_HD static inline uint8_t kt_tile_byte(int first, int last) { return (uint8_t)(first | last << 2); }
KQ_HD static inline int kt_byte_first(uint8_t b) { return b & 3; }
KQ_HD static inline int kt_byte_last(uint8_t b) { return (b >> 2) & 3; }

// a round of the seam walk in front of tile `hi` of a contig whose first tile is t0 (t0 < hi): lane `lane` looks at tile hi - 1 - lane -> its
// last type, none in front of t0.  Reads tb[t] with t0 <= t < hi only.
KQ_HD static inline int kt_seam_look(const uint8_t *tb, int64_t t0, int64_t hi, int lane)
{
    const int64_t t = hi - 1 - lane;
    return t >= t0 ? kt_byte_last(tb[t]) : KT_NONE;
}

}  // namespace
