// kset.hpp — the k-mer set object (cornetto_kset_*) and its tile table, shared by kqv.hip (`cornetto qv`: the plain set) and ktrio.hip
// (`cornetto trioeval`: the tagged set) and kcount.hip (the counted set of either, from reads).  A set is either plain or tagged, decided by its
// first add; the other family's calls are refused.  A counted set (cornetto_kset_open_counted) is KSET_COUNTED until its seal makes it plain or
// tagged; `counted` stays set, and the adds refuse it for good.
#pragma once
#include <new>

#include "common.hpp"
#include "kqv.hpp"
#include "tiles.hpp"

enum { KSET_UNSET = -1, KSET_PLAIN = 0, KSET_TAGGED = 1, KSET_COUNTED = 2 };

struct cornetto_kset {
    int32_t k = 0;
    int64_t slots = 0;
    uint64_t *d_tab = nullptr;
    unsigned long long *d_stat = nullptr;   // [0] positions inserted, [1] distinct, [2] overflow, [3], [4] solid keys per channel (kq_seal)
    uint32_t *d_cnt = nullptr;              // a counted set before its seal: channels * slots counts, count[ch * slots + slot]
    uint32_t *d_cop = nullptr;              // ... of one channel, from its first kset_copies: a byte of copies per slot, four to a word (kqv.hpp)
    bool copied = false;                    // kset_copies has run: the table may hold assembly-only keys, kset_count is refused
    int32_t channels = 0;                   // 0: not a counted set
    bool counted = false;                   // opened by cornetto_kset_open_counted (also after the seal)
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

// cornetto_kset_open (channels = 0) and cornetto_kset_open_counted (1 or 2): the object, the table emptied and the counts zeroed on the stream
inline int kq_open(cornetto_accel_t *h, const char *who, int32_t k, int64_t slots, int32_t channels, cornetto_kset_t **out)
{
    if (!h || !out || slots < 1) return cn_fail(h, CORNETTO_E_ARG, "%s: bad argument", who);
    *out = nullptr;
    if (!kq_k_ok(k)) return cn_fail(h, CORNETTO_E_UNSUPPORTED, "%s: k = %d; k is odd, 11 to 31", who, (int)k);
    CN_HIP(h, hipSetDevice(h->device));
    if (slots > ((int64_t)1 << 58)) return cn_fail(h, CORNETTO_E_NOMEM, "%s: a table of %lld slots wants more than 2^61 bytes", who, (long long)slots);
    const size_t per = 8 + 4 * (size_t)channels;
    cornetto_kset_t *s = new (std::nothrow) cornetto_kset;
    if (!s) return cn_fail(h, CORNETTO_E_NOMEM, "%s: host allocation failed", who);
    s->k = k;
    s->slots = slots;
    s->stats[2] = slots;
    s->channels = channels;
    s->counted = channels > 0;
    if (channels) s->mode = KSET_COUNTED;
    const size_t cnt_bytes = (size_t)slots * 4 * (size_t)channels;
    if (hipMalloc((void **)&s->d_tab, (size_t)slots * 8) != hipSuccess || (channels && hipMalloc((void **)&s->d_cnt, cnt_bytes) != hipSuccess) ||
        hipMalloc((void **)&s->d_stat, 64) != hipSuccess) {
        (void)hipGetLastError();
        if (s->d_tab) (void)hipFree(s->d_tab);
        if (s->d_cnt) (void)hipFree(s->d_cnt);
        delete s;
        return cn_fail(h, CORNETTO_E_NOMEM, "%s: a table of %lld slots wanted %lld bytes of device memory", who, (long long)slots, (long long)slots * (long long)per);
    }
    // every slot empty and every count 0, whatever the memory held: on the handle's stream, in front of the first insert
    const hipError_t e1 = hipMemsetAsync(s->d_tab, 0xFF, (size_t)slots * 8, h->stream), e2 = hipMemsetAsync(s->d_stat, 0, 64, h->stream),
                     e3 = channels ? hipMemsetAsync(s->d_cnt, 0, cnt_bytes, h->stream) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipFree(s->d_tab);
        (void)hipFree(s->d_stat);
        if (s->d_cnt) (void)hipFree(s->d_cnt);
        delete s;
        return cn_fail(h, CORNETTO_E_HIP, "%s: the table could not be cleared", who);
    }
    *out = s;
    return CORNETTO_OK;
}

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
