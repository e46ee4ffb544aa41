// kset.hpp — the k-mer set object (cornetto_kset_*) and its tile table, shared by kqv.hip (`cornetto qv`: the plain set) and ktrio.hip
// (`cornetto trioeval`: the tagged set).  A set is either plain or tagged, decided by its first add; the other family's calls are refused.
#pragma once
#include "common.hpp"
#include "kqv.hpp"
#include "tiles.hpp"

enum { KSET_UNSET = -1, KSET_PLAIN = 0, KSET_TAGGED = 1 };

struct cornetto_kset {
    int32_t k = 0;
    int64_t slots = 0;
    uint64_t *d_tab = nullptr;
    unsigned long long *d_stat = nullptr;   // [0] positions inserted, [1] distinct, [2] overflow
    int64_t stats[3] = {0, 0, 0};           // host copy of [0], [1]; [2] = slots
    bool dead = false;                      // the table overflowed
    int mode = KSET_UNSET;                  // plain (kset_add / kset_query) or tagged (kset_add_tag / kset_phase)
    // the tile table of the last assembly seen (rebuilt per call: a function of the lengths alone)
    CnPrefix pref;
    int2 *d_tiles = nullptr;
    size_t tiles_cap = 0;
};

namespace {

struct KqTileFill {
    int2 *out;
    __device__ void operator()(int64_t t, int c, int64_t j) const { out[t] = make_int2(c, (int)(j * KQ_TILE)); }
};

// the tile table of `a` in the set's own buffers -> the number of tiles, or a negative status
inline int64_t kq_tiles(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a)
{
    const int64_t nt = cntiles::prefix(h, s->pref, a->n, [&](int32_t c) { return ((int64_t)a->len[c] + KQ_TILE - 1) / KQ_TILE; });
    if (nt < 0) return cn_fail(h, CORNETTO_E_NOMEM, "kset: device allocation failed");
    if (nt > 0x7fffffffll) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "kset: too many tiles");
    if (nt == 0) return 0;
    if (s->tiles_cap < (size_t)nt) {
        if (s->d_tiles) (void)hipFree(s->d_tiles);
        s->d_tiles = nullptr;
        s->tiles_cap = 0;
        if (cn_obj_malloc(h, (void **)&s->d_tiles, (size_t)nt * sizeof(int2)) != hipSuccess) {
            (void)hipGetLastError();
            return cn_fail(h, CORNETTO_E_NOMEM, "kset: device allocation failed");
        }
        s->tiles_cap = (size_t)nt;
    }
    cntiles::fill<<<dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, h->stream>>>(s->pref.dev, a->n, nt, KqTileFill{s->d_tiles});
    if (hipGetLastError() != hipSuccess) return cn_fail(h, CORNETTO_E_HIP, "kset: the tile table could not be launched");
    return nt;
}

}  // namespace
