/* kmer.h — the canonical k-mers of a record on the host, for the --accel=no paths of `cornetto qv` and `cornetto trioeval`: the rule that
 * include/cornetto_accel.h states for `qv` (base codes, positions that hold a k-mer, min(fwd, rc)), one byte at a time, and the hash of the host
 * tables.  The device has the same rule in csrc/kqv.hpp. */
#ifndef CORNETTO_CLI_KMER_H
#define CORNETTO_CLI_KMER_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cornetto_accel.h"

static inline int cli_kmer_code(unsigned char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

/* the finaliser of MurmurHash3 (public domain) */
static inline uint64_t cli_kmer_mix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

typedef struct {
    uint64_t fwd, rc, mask;
    int valid, k;
} cli_kroll_t;

static inline void cli_kroll_init(cli_kroll_t *r, int k)
{
    r->fwd = r->rc = 0;
    r->mask = ((uint64_t)1 << (2 * k)) - 1;
    r->valid = 0;
    r->k = k;
}

/* the next byte of the record; 1 when a k-mer ends at it (it begins k - 1 bytes in front): *key = its canonical code */
static inline int cli_kroll_push(cli_kroll_t *r, unsigned char byte, uint64_t *key)
{
    const int c = cli_kmer_code(byte);
    if (c > 3) {
        r->valid = 0;
        return 0;
    }
    r->fwd = ((r->fwd << 2) | (uint64_t)c) & r->mask;
    r->rc = (r->rc >> 2) | ((uint64_t)(3 - c) << (2 * (r->k - 1)));
    if (r->valid < r->k) ++r->valid;
    if (r->valid < r->k) return 0;
    *key = r->fwd < r->rc ? r->fwd : r->rc;
    return 1;
}

/* ---- the counted table of `qv -r` and `trioeval --pat-reads / --mat-reads` on the host (the rule: include/cornetto_accel.h, "Counted k-mer sets"):
 * a key array with linear probing, ~0 = empty, and channels * slots counts beside it, count[ch * slots + slot], saturating at the cap.  Sealing
 * rewrites the key array in place into the plain (one channel) or the tagged (two: key | tag << 62) table that the host lookups of qv_main.c and
 * trioeval_main.c walk, a key that is solid nowhere becoming the tombstone ~0 - 1: no key equals it, whole or under the 62-bit key mask (the
 * proof stands in csrc/kqv.hpp), and the lookups stop at ~0 only. */
#define CLI_KCOUNT_CAP CORNETTO_KSET_COUNT_CAP
#define CLI_KCOUNT_BINS CORNETTO_KSET_HIST_BINS

#define CLI_KCOUNT_CN_BINS CORNETTO_KSET_CN_BINS

typedef struct {
    uint64_t *tab;
    uint32_t *cnt;
    uint8_t *cop;        /* one channel, from the first cli_kcount_copy(): the copies of the slot's key in the assembly, saturating at CN_BINS - 1 */
    int64_t slots, pos, distinct;
    int channels;
} cli_kcount_t;

/* 0, or -1 when the slots * (8 + 4 * channels) bytes cannot be had */
static inline int cli_kcount_init(cli_kcount_t *t, int64_t slots, int channels)
{
    memset(t, 0, sizeof(*t));
    t->slots = slots;
    t->channels = channels;
    if ((uint64_t)slots > SIZE_MAX / 16) return -1;
    t->tab = (uint64_t *)malloc((size_t)slots * 8);
    t->cnt = (uint32_t *)calloc((size_t)slots * (size_t)channels, 4);
    if (!t->tab || !t->cnt) {
        free(t->tab);
        free(t->cnt);
        t->tab = NULL;
        t->cnt = NULL;
        return -1;
    }
    memset(t->tab, 0xFF, (size_t)slots * 8);
    return 0;
}

/* one occurrence of `key` in channel `ch`: 0, or -1 when the table has no room */
static inline int cli_kcount_add(cli_kcount_t *t, uint64_t key, int ch)
{
    const uint64_t slots = (uint64_t)t->slots;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (t->tab[s] == ~(uint64_t)0) {
            t->tab[s] = key;
            t->distinct++;
        }
        if (t->tab[s] == key) {
            uint32_t *c = t->cnt + (uint64_t)ch * slots + s;
            if (*c < CLI_KCOUNT_CAP) ++*c;
            t->pos++;
            return 0;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
    return -1;
}

/* hist[0 .. CLI_KCOUNT_BINS) of channel `ch` */
static inline void cli_kcount_hist(const cli_kcount_t *t, int ch, int64_t *hist)
{
    memset(hist, 0, CLI_KCOUNT_BINS * sizeof(int64_t));
    for (int64_t i = 0; i < t->slots; ++i) {
        const uint32_t c = t->cnt[(int64_t)ch * t->slots + i];
        if (c) hist[c < CLI_KCOUNT_BINS - 1 ? c : CLI_KCOUNT_BINS - 1]++;
    }
}

/* one occurrence of `key` in the assembly ("Completeness and copy-number spectrum" in include/cornetto_accel.h): a key the table does not hold
 * takes a slot with count 0 and is no distinct key of the reads.  0, or -1 when the table has no room or the bytes cannot be had */
static inline int cli_kcount_copy(cli_kcount_t *t, uint64_t key)
{
    const uint64_t slots = (uint64_t)t->slots;
    if (!t->cop && !(t->cop = (uint8_t *)calloc((size_t)slots, 1))) return -1;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (t->tab[s] == ~(uint64_t)0) t->tab[s] = key;
        if (t->tab[s] == key) {
            if (t->cop[s] < CLI_KCOUNT_CN_BINS - 1) ++t->cop[s];
            return 0;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
    return -1;
}

static inline void cli_kcount_copies_clear(cli_kcount_t *t)
{
    if (t->cop) memset(t->cop, 0, (size_t)t->slots);
}

/* spec[a * CLI_KCOUNT_BINS + c] of channel `ch` and totals = {solid, found} for the threshold m */
static inline void cli_kcount_spectrum(const cli_kcount_t *t, int ch, int m, int64_t *spec, int64_t *totals)
{
    memset(spec, 0, (size_t)CLI_KCOUNT_CN_BINS * CLI_KCOUNT_BINS * sizeof(int64_t));
    totals[0] = totals[1] = 0;
    for (int64_t i = 0; i < t->slots; ++i) {
        const uint32_t c = t->cnt[(int64_t)ch * t->slots + i];
        const int a = t->cop ? t->cop[i] : 0;
        if (!c && !a) continue;
        spec[(int64_t)a * CLI_KCOUNT_BINS + (c < CLI_KCOUNT_BINS - 1 ? c : CLI_KCOUNT_BINS - 1)]++;
        if (c && c >= (uint32_t)m) {
            totals[0]++;
            totals[1] += a != 0;
        }
    }
}

/* the seal: solid[ch] = keys with count >= m[ch]; the counts are freed, t->tab is the plain or the tagged table */
static inline void cli_kcount_seal(cli_kcount_t *t, const int *m, int64_t *solid)
{
    for (int ch = 0; ch < t->channels; ++ch) solid[ch] = 0;
    for (int64_t i = 0; i < t->slots; ++i) {
        if (t->tab[i] == ~(uint64_t)0) continue;
        uint64_t tag = 0;
        for (int ch = 0; ch < t->channels; ++ch)
            if (t->cnt[(int64_t)ch * t->slots + i] >= (uint32_t)m[ch]) {
                tag |= (uint64_t)1 << ch;
                solid[ch]++;
            }
        if (!tag) t->tab[i] = ~(uint64_t)0 - 1;
        else if (t->channels == 2) t->tab[i] |= tag << 62;
    }
    free(t->cnt);
    t->cnt = NULL;
    free(t->cop);
    t->cop = NULL;
}

/* an upper bound of the positions of a file of parental or truth records: the bytes of a plain regular file, else the sum of the record lengths
 * of one pass over it; -1: a FIFO or `-`, which can be read only once (qv_main.c) */
int64_t cli_kmer_file_bound(const char *path);

#endif
