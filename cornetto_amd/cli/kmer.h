/* kmer.h — the canonical k-mers of a record on the host, for the --accel=no paths of `cornetto qv` and `cornetto trioeval`: the rule that
 * include/cornetto_accel.h states for `qv` (base codes, positions that hold a k-mer, min(fwd, rc)), one byte at a time, and the hash of the host
 * tables.  The device has the same rule in csrc/kqv.hpp. */
#ifndef CORNETTO_CLI_KMER_H
#define CORNETTO_CLI_KMER_H

#include <stdint.h>

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

/* an upper bound of the positions of a file of parental or truth records: the bytes of a plain regular file, else the sum of the record lengths
 * of one pass over it; -1: a FIFO or `-`, which can be read only once (qv_main.c) */
int64_t cli_kmer_file_bound(const char *path);

#endif
