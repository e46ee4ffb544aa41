/* host_backend.c — the product's own HOST path of the panel scans: plain sequential C99, no device, no library call.
 *
 * Selected explicitly — `--accel=no` (the switch the reference left for this: src/boringbits_main.c:627-632,
 * src/cornetto.c:323-325) or CORNETTO_ACCEL=no for the sub-commands that have no such option — never silently: without
 * that choice a box without a usable GPU still gets the "cannot open HIP device" exit.  It exists so that the binary runs
 * BASELINE's configuration 1 ("CPU only ... plumbing, no GPU") as written and so that `--accel=no` means what it says.
 * It is not a tuned CPU implementation and not the timed baseline of bench.py (that is the unmodified reference).
 *
 * Every unit takes and returns the C ABI's record types (include/cornetto_accel.h), so the sub-command mains print the
 * host results with the code that prints the device results.  Written for this file; nothing under oracle/ is used. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "cli.h"

/* ------------------------------------------------------------------------------------------------ the switch */
static int g_host = -1;

int cli_host_mode(void)
{
    if (g_host < 0) {
        const char *e = getenv("CORNETTO_ACCEL");
        g_host = e && (!strcmp(e, "no") || !strcmp(e, "n") || !strcmp(e, "0") || !strcmp(e, "cpu") || !strcmp(e, "host"));
    }
    return g_host;
}

void cli_host_set(int on) { g_host = on ? 1 : 0; }

/* ------------------------------------------------------------------------------------------------ telofind
 * src/find_telomere.c:44-74 on one record: the contig is compared upper-cased (:76-81; the motif is taken as given),
 * runs are greedy and never overlap (:52-57), strand 0 = the motif, then strand 1 = its reverse complement (:61-72). */
typedef struct {
    cornetto_hit_t *a;
    int64_t n, cap;
} hitbuf_t;

static inline uint8_t fold(uint8_t c) { return (uint8_t)(c >= 'a' && c <= 'z' ? c - 32 : c); }

static inline int motif_at(const uint8_t *s, const uint8_t *pat, int64_t k)
{
    for (int64_t j = 0; j < k; ++j)
        if (fold(s[j]) != pat[j]) return 0;
    return 1;
}

static void strand_runs(const uint8_t *s, int64_t n, const uint8_t *pat, int64_t k, int32_t ctg, int32_t strand, hitbuf_t *out)
{
    int64_t p = 0;
    while (p + k <= n) {
        while (p + k <= n && !motif_at(s + p, pat, k)) ++p;      /* the next occurrence at or behind p (:49) */
        if (p + k > n) break;
        int64_t e = p + k;
        while (e + k <= n && motif_at(s + e, pat, k)) e += k;     /* :52-55 */
        if (out->n == out->cap) {
            out->cap = out->cap ? out->cap * 2 : 256;
            out->a = (cornetto_hit_t *)cli_xrealloc(out->a, (size_t)out->cap * sizeof(*out->a));
        }
        out->a[out->n].ctg = ctg;
        out->a[out->n].strand = strand;
        out->a[out->n].start = (int32_t)p;
        out->a[out->n].end = (int32_t)e;
        out->n++;
        p = e + 1;                                                /* :57 */
    }
}

void cli_host_telofind(const uint8_t *seq, int64_t len, const char *motif, int32_t ctg, cornetto_hit_t **hits, int64_t *n_hits, int64_t *cap_hits)
{
    hitbuf_t b = {*hits, *n_hits, *cap_hits};
    const int64_t k = (int64_t)strlen(motif);
    const uint8_t *nul = (const uint8_t *)memchr(seq, 0, (size_t)len);   /* strstr() of the reference ends at a NUL byte */
    const int64_t n = nul ? (int64_t)(nul - seq) : len;
    if (k > 0 && k <= n) {
        uint8_t *rc = (uint8_t *)cli_xmalloc((size_t)k + 1);
        for (int64_t i = 0; i < k; ++i) {                         /* :24-42: A<->T, C<->G, anything else as it is */
            const char c = motif[k - 1 - i];
            rc[i] = (uint8_t)(c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c);
        }
        strand_runs(seq, n, (const uint8_t *)motif, k, ctg, 0, &b);
        strand_runs(seq, n, rc, k, ctg, 1, &b);
        free(rc);
    }
    *hits = b.a;
    *n_hits = b.n;
    *cap_hits = b.cap;
}

/* ------------------------------------------------------------------------------------------------ telowin
 * src/telomere_windows.c:69-79 (marks) and :28-43 (windows): one bit per base, windows of 1000 every 200. */
static inline int64_t bits_in(const uint64_t *w, int64_t a, int64_t b) /* set bits in [a, b) */
{
    if (a >= b) return 0;
    const int64_t wa = a >> 6, wb = (b - 1) >> 6;
    const uint64_t ma = ~0ull << (a & 63), mb = ~0ull >> (63 - ((b - 1) & 63));
    if (wa == wb) return __builtin_popcountll(w[wa] & ma & mb);
    int64_t c = __builtin_popcountll(w[wa] & ma) + __builtin_popcountll(w[wb] & mb);
    for (int64_t i = wa + 1; i < wb; ++i) c += __builtin_popcountll(w[i]);
    return c;
}

static inline void bits_set(uint64_t *w, int64_t a, int64_t b) /* [a, b) */
{
    if (a >= b) return;
    const int64_t wa = a >> 6, wb = (b - 1) >> 6;
    const uint64_t ma = ~0ull << (a & 63), mb = ~0ull >> (63 - ((b - 1) & 63));
    if (wa == wb) {
        w[wa] |= ma & mb;
        return;
    }
    w[wa] |= ma;
    for (int64_t i = wa + 1; i < wb; ++i) w[i] = ~0ull;
    w[wb] |= mb;
}

void cli_host_telowin(const cornetto_hit_t *hits, int64_t n_hits, const int32_t *lens, int32_t n_ctg, double thr_adj, cornetto_win_t **wins, int64_t *n_wins)
{
    cornetto_win_t *o = NULL;
    int64_t n = 0, cap = 0, h = 0;
    for (int32_t c = 0; c < n_ctg; ++c) {
        const int64_t len = lens[c];
        uint64_t *mark = (uint64_t *)calloc((size_t)(len / 64 + 2), sizeof(uint64_t));
        if (!mark) {
            CLI_ERROR("%s", "out of memory");
            exit(EXIT_FAILURE);
        }
        for (; h < n_hits && hits[h].ctg == c; ++h) bits_set(mark, hits[h].start, hits[h].end);
        for (int64_t i = 0; i <= len; i += 200) {                                  /* :31 */
            const int64_t hi = i + 1000 < len ? i + 1000 : len;
            const int64_t car = bits_in(mark, i, hi);                              /* :33-35 */
            const int64_t den = i + 1000 < len ? 1000 : len - i;                   /* :36 */
            if ((double)car / (double)den >= thr_adj) {                            /* :37 (0 / 0 = NaN: no window) */
                if (n == cap) {
                    cap = cap ? cap * 2 : 256;
                    o = (cornetto_win_t *)cli_xrealloc(o, (size_t)cap * sizeof(*o));
                }
                o[n].ctg = c;
                o[n].start = (int32_t)i;
                o[n].end = (int32_t)(i + den);
                o[n].car = (int32_t)car;
                ++n;
            }
            if (i + 1000 >= len) break;                                            /* :40 */
        }
        free(mark);
    }
    *wins = o;
    *n_wins = n;
}

/* ------------------------------------------------------------------------------------------------ telostats
 * scripts/telostats.sh:35-47 on one record, step by step as the script's pipeline does it: the runs (telofind), the windows (telowin),
 * `bedtools merge -d merge_dist` as a sweep over the windows in start order, then `bedtools intersect -wa` against the record's end
 * intervals (:44) — a region once per end interval it shares a base with.  Deliberately the sequential form, not the run-length rule of
 * the device stage (csrc/telostats.hip): a second, independent statement of the same rows. */
static void ends_push(cornetto_ivl_t **rows, int64_t *n, int64_t *cap, int32_t ctg, int64_t s, int64_t e, const int64_t (*iv)[2], int n_iv)
{
    for (int k = 0; k < n_iv; ++k) {
        if (!(s < iv[k][1] && e > iv[k][0])) continue;             /* no base in common with this end interval */
        if (*n == *cap) {
            *cap = *cap ? *cap * 2 : 64;
            *rows = (cornetto_ivl_t *)cli_xrealloc(*rows, (size_t)*cap * sizeof(**rows));
        }
        (*rows)[*n].ctg = ctg;
        (*rows)[*n].start = (int32_t)s;
        (*rows)[*n].finish = (int32_t)e;
        ++*n;
    }
}

void cli_host_telo_ends(const uint8_t *seq, int64_t len, const char *motif, double thr_adj, int32_t merge_dist, int32_t ends, int32_t ctg,
                        cornetto_ivl_t **rows, int64_t *n_rows, int64_t *cap_rows)
{
    cornetto_hit_t *hits = NULL;
    int64_t n_hits = 0, cap_hits = 0, n_wins = 0;
    cornetto_win_t *wins = NULL;
    const int32_t len32 = (int32_t)len;
    cli_host_telofind(seq, len, motif, 0, &hits, &n_hits, &cap_hits);
    cli_host_telowin(hits, n_hits, &len32, 1, thr_adj, &wins, &n_wins);
    int64_t iv[2][2] = {{0, len}, {0, 0}};                         /* :44 */
    int n_iv = 1;
    if (len > 2 * (int64_t)ends) {
        iv[0][1] = ends;
        iv[1][0] = len - ends;
        iv[1][1] = len;
        n_iv = 2;
    }
    int64_t s = 0, e = -1;                                         /* the region being grown (none yet: e < 0) */
    for (int64_t i = 0; i < n_wins; ++i) {
        if (e >= 0 && wins[i].start <= e + merge_dist) {           /* bedtools merge -d: at most merge_dist behind the end so far */
            if (wins[i].end > e) e = wins[i].end;
            continue;
        }
        if (e >= 0) ends_push(rows, n_rows, cap_rows, ctg, s, e, (const int64_t (*)[2])iv, n_iv);
        s = wins[i].start;
        e = wins[i].end;
    }
    if (e >= 0) ends_push(rows, n_rows, cap_rows, ctg, s, e, (const int64_t (*)[2])iv, n_iv);
    free(hits);
    free(wins);
}

/* ------------------------------------------------------------------------------------------------ sdust
 * src/sdust/sdust.c:130-160 on one record, base by base.  State: the FIFO of the last <= W - 2 three-letter words with
 * its pair score (rw), the suffix of it in which no word occurs more than 2T/10 times (length L, pair score rv), the
 * perfect intervals found so far that may still grow (P, by descending start), the result list. */
typedef struct {
    int32_t start, finish, r, l;
} perfect_t;

typedef struct {
    uint8_t *fifo;
    int cap, head, n;
    int cw[64], cv[64];
    int rw, rv, L;
    perfect_t *P;
    int nP, capP;
    cornetto_ivl_t *out;
    int64_t n_out, cap_out, first_out; /* first_out: where this record's intervals begin (merging never reaches further back) */
    int32_t ctg;
} dust_t;

static inline int dust_word(const dust_t *d, int i) { return d->fifo[(d->head + i) % d->cap]; }

/* :88-102: the interval with the smallest start has left the window for good -> into the result, merged with the last
 * one when they overlap or touch; then every perfect interval that starts in front of `start` is dropped */
static void dust_retire(dust_t *d, int start)
{
    if (d->nP == 0 || d->P[d->nP - 1].start >= start) return;
    const perfect_t *p = &d->P[d->nP - 1];
    if (d->n_out > d->first_out && p->start <= d->out[d->n_out - 1].finish) {
        if (p->finish > d->out[d->n_out - 1].finish) d->out[d->n_out - 1].finish = p->finish;
    } else {
        if (d->n_out == d->cap_out) {
            d->cap_out = d->cap_out ? d->cap_out * 2 : 256;
            d->out = (cornetto_ivl_t *)cli_xrealloc(d->out, (size_t)d->cap_out * sizeof(*d->out));
        }
        d->out[d->n_out].ctg = d->ctg;
        d->out[d->n_out].start = p->start;
        d->out[d->n_out].finish = p->finish;
        d->n_out++;
    }
    while (d->nP > 0 && d->P[d->nP - 1].start < start) d->nP--;
}

/* :66-86 */
static void dust_push(dust_t *d, int t, int T, int W)
{
    if (d->n >= W - 2) {
        const int x = d->fifo[d->head];
        d->head = (d->head + 1) % d->cap;
        d->n--;
        d->rw -= --d->cw[x];
        if (d->L > d->n) {
            d->L--;
            d->rv -= --d->cv[x];
        }
    }
    d->fifo[(d->head + d->n) % d->cap] = (uint8_t)t;
    d->n++;
    d->L++;
    d->rw += d->cw[t]++;
    d->rv += d->cv[t]++;
    if (d->cv[t] * 10 > T << 1) {
        int x;
        do {
            x = dust_word(d, d->n - d->L);
            d->rv -= --d->cv[x];
            d->L--;
        } while (x != t);
    }
}

/* :104-128: every suffix of the window that is longer than the L-suffix, from short to long */
static void dust_perfect(dust_t *d, int T, int start)
{
    int c[64];
    memcpy(c, d->cv, sizeof(c));
    int r = d->rv, best_r = 0, best_l = 0;
    for (int i = d->n - d->L - 1; i >= 0; --i) {
        const int t = dust_word(d, i);
        r += c[t]++;
        const int l = d->n - i - 1;
        if (r * 10 <= T * l) continue;
        int j = 0;
        for (; j < d->nP && d->P[j].start >= i + start; ++j)
            if (best_r == 0 || d->P[j].r * best_l > best_r * d->P[j].l) {
                best_r = d->P[j].r;
                best_l = d->P[j].l;
            }
        if (best_r == 0 || r * best_l >= best_r * l) {
            best_r = r;
            best_l = l;
            if (d->nP == d->capP) {
                d->capP = d->capP ? d->capP * 2 : 64;
                d->P = (perfect_t *)cli_xrealloc(d->P, (size_t)d->capP * sizeof(*d->P));
            }
            memmove(d->P + j + 1, d->P + j, (size_t)(d->nP - j) * sizeof(*d->P));
            d->nP++;
            d->P[j].start = i + start;
            d->P[j].finish = d->n + 2 + start;
            d->P[j].r = r;
            d->P[j].l = l;
        }
    }
}

static inline int base_code(uint8_t c) /* seq_nt4_table, :23-40: ACGT in either case, the bytes 0..3 themselves, 4 otherwise */
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return c < 4 ? c : 4;
    }
}

int cli_host_sdust(const uint8_t *seq, int64_t len, int T, int W, int32_t ctg, cornetto_ivl_t **ivls, int64_t *n_ivls, int64_t *cap_ivls)
{
    if (W < 3 || W > 1026 || T < 0 || T > (1 << 20) || len > 0x7fffffffLL) return -1;   /* (the limits of the device path) */
    dust_t d;
    memset(&d, 0, sizeof(d));
    d.cap = W + 2;
    d.fifo = (uint8_t *)cli_xmalloc((size_t)d.cap);
    d.out = *ivls;
    d.n_out = d.first_out = *n_ivls;
    d.cap_out = *cap_ivls;
    d.ctg = ctg;
    int l = 0;
    unsigned t = 0;
    for (int64_t i = 0; i <= len; ++i) {                                  /* :141: one step past the end flushes P */
        const int b = i < len ? base_code(seq[i]) : 4;
        if (b < 4) {
            ++l;
            t = (t << 2 | (unsigned)b) & 63u;
            if (l >= 3) {
                const int start = (l - W > 0 ? l - W : 0) + (int)(i + 1 - l);          /* :146 */
                dust_retire(&d, start);
                dust_push(&d, (int)t, T, W);
                if (d.rw * 10 > d.L * T) dust_perfect(&d, T, start);                  /* :149 */
            }
        } else {
            int start = (l - W + 1 > 0 ? l - W + 1 : 0) + (int)(i + 1 - l);            /* :152 */
            while (d.nP) dust_retire(&d, start++);                                     /* :153 */
            l = 0;                                                                     /* :154: the words and their counts stay */
            t = 0;
        }
    }
    free(d.fifo);
    free(d.P);
    *ivls = d.out;
    *n_ivls = d.n_out;
    *cap_ivls = d.cap_out;
    return 0;
}

/* ------------------------------------------------------------------------------------------------ get_depths
 * src/boringbits_main.c:180-301: the two per-base bedgraphs read in lock-step the way fscanf("%s\t%d\t%d\t%d\n") reads
 * them — a record is four white-space separated tokens whatever the lines look like — with the reference's checks in
 * its order.  A small buffered byte stream with the two conversions, not fscanf: no 10 000-byte name buffer to overrun. */
typedef struct {
    FILE *f;
    unsigned char *buf;
    size_t n, at;
    int eof;
} bgs_t;

static inline int bgs_peek(bgs_t *s)
{
    if (s->at == s->n) {
        if (s->eof) return -1;
        s->n = fread(s->buf, 1, 1 << 20, s->f);
        s->at = 0;
        if (s->n == 0) {
            s->eof = 1;
            return -1;
        }
    }
    return s->buf[s->at];
}

static inline int is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

static void bgs_skip_space(bgs_t *s)
{
    int c;
    while ((c = bgs_peek(s)) >= 0 && is_space(c)) s->at++;
}

/* %s: 1 converted, 0 end of input */
static int bgs_string(bgs_t *s, cli_str_t *name)
{
    bgs_skip_space(s);
    int c = bgs_peek(s);
    if (c < 0) return 0;
    name->l = 0;
    while ((c = bgs_peek(s)) >= 0 && !is_space(c)) {
        if (name->l + 2 > name->m) {
            name->m = name->m ? name->m * 2 : 64;
            name->s = (char *)cli_xrealloc(name->s, name->m);
        }
        name->s[name->l++] = (char)c;
        s->at++;
    }
    name->s[name->l] = 0;
    return 1;
}

/* %d: 1 converted, 0 no number here (or end of input) */
static int bgs_int(bgs_t *s, int *v)
{
    bgs_skip_space(s);
    int c = bgs_peek(s), neg = 0;
    if (c == '-' || c == '+') {
        neg = c == '-';
        s->at++;
        c = bgs_peek(s);
    }
    if (c < '0' || c > '9') return 0;
    long long x = 0;
    while ((c = bgs_peek(s)) >= '0' && c <= '9') {
        if (x < (1ll << 40)) x = x * 10 + (c - '0');
        s->at++;
    }
    *v = (int)(neg ? -x : x);
    return 1;
}

/* one record -> converted fields (4 = a record; 0 with nothing read = end of the file, what fscanf reports as EOF) */
static int bgs_record(bgs_t *s, cli_str_t *name, int *st, int *end, int *depth)
{
    if (!bgs_string(s, name)) return -1;
    if (!bgs_int(s, st)) return 1;
    if (!bgs_int(s, end)) return 2;
    if (!bgs_int(s, depth)) return 3;
    return 4;
}

void cli_host_get_depths(FILE *ft, FILE *fq, cli_host_cov_t *out)
{
    bgs_t a = {ft, (unsigned char *)cli_xmalloc(1 << 20), 0, 0, 0}, b = {fq, (unsigned char *)cli_xmalloc(1 << 20), 0, 0, 0};
    cli_str_t na = {0, 0, 0}, nb = {0, 0, 0};
    memset(out, 0, sizeof(*out));
    int32_t cap_ctg = 0;
    int64_t cap_pos = 0;
    int prev_pos = 0;
    double tot = 0, tot_mq = 0, tot_len = 0;
    for (;;) {
        int st1, end1, d1, st2, end2, d2;
        int r = bgs_record(&a, &na, &st1, &end1, &d1);
        if (r < 0) break;                                                              /* :205-207 */
        if (r != 4) {
            CLI_ERROR("The depth files should have 4 columns. Had %d.", r);            /* :209-212 */
            exit(EXIT_FAILURE);
        }
        r = bgs_record(&b, &nb, &st2, &end2, &d2);
        if (r < 0) {
            CLI_ERROR("%s", "The two files are not in the same order");               /* :214-217 */
            exit(EXIT_FAILURE);
        }
        if (r != 4) {
            CLI_ERROR("The depth files should have 4 columns. Had %d.", r);            /* :219-222 */
            exit(EXIT_FAILURE);
        }
        if (strcmp(na.s, nb.s) != 0 || st1 != st2 || end1 != end2) {
            CLI_ERROR("%s", "The two files are not in the same order");               /* :224-227 */
            exit(EXIT_FAILURE);
        }
        if (out->n_ctg == 0 || strcmp(na.s, out->names[out->n_ctg - 1]) != 0) {       /* :229-246 (prev_ctg starts as "") */
            if (out->n_ctg == 0 && na.l == 0) { /* cannot happen: %s never converts an empty token */ }
            if (out->n_ctg == cap_ctg) {
                cap_ctg = cap_ctg ? cap_ctg * 2 : 256;
                out->names = (char **)cli_xrealloc(out->names, (size_t)cap_ctg * sizeof(char *));
                out->lens = (int32_t *)cli_xrealloc(out->lens, (size_t)cap_ctg * sizeof(int32_t));
                out->first = (int64_t *)cli_xrealloc(out->first, ((size_t)cap_ctg + 1) * sizeof(int64_t));
            }
            out->names[out->n_ctg] = cli_xstrdup(na.s);
            out->lens[out->n_ctg] = 0;
            out->first[out->n_ctg] = out->n_pos;
            out->n_ctg++;
            prev_pos = 0;
        } else {
            if (prev_pos + 1 != st1) {
                CLI_ERROR("The depth files should be incremantal at one base resolution. Found %d to %d", prev_pos, st1);   /* :249-252 */
                exit(EXIT_FAILURE);
            }
            prev_pos++;
        }
        if (st1 + 1 != end1) {
            CLI_ERROR("The depth files should have end=start+1. Found %d to %d", st1, end1);   /* :256-259 */
            exit(EXIT_FAILURE);
        }
        if (d1 > 65535) {                                                             /* :261-268 */
            d1 = 65535;
            out->n_clamped++;
        }
        if (d2 > 65535) {
            d2 = 65535;
            out->n_clamped++;
        }
        if (out->lens[out->n_ctg - 1] == 0x7fffffff) {
            CLI_ERROR("contig %s has more than 2^31-1 positions", na.s);
            exit(EXIT_FAILURE);
        }
        if (out->n_pos == cap_pos) {
            cap_pos = cap_pos ? cap_pos * 2 : 1 << 20;
            out->depth = (uint16_t *)cli_xrealloc(out->depth, (size_t)cap_pos * sizeof(uint16_t));
            out->mq = (uint16_t *)cli_xrealloc(out->mq, (size_t)cap_pos * sizeof(uint16_t));
        }
        out->depth[out->n_pos] = (uint16_t)d1;                                        /* (a negative value wraps, as there) */
        out->mq[out->n_pos] = (uint16_t)d2;
        out->n_pos++;
        out->lens[out->n_ctg - 1]++;
        tot += d1;                                                                    /* :283-285 */
        tot_mq += d2;
        tot_len++;
    }
    if (out->first) out->first[out->n_ctg] = out->n_pos;
    out->sum_depth = tot;
    out->sum_mq = tot_mq;
    out->positions = tot_len;
    free(a.buf);
    free(b.buf);
    free(na.s);
    free(nb.s);
}

/* ------------------------------------------------------------------------------------------------ get_depths, run-length files
 * `--runs` (an extension, see boringbits_main.c): a record `name s e v` stands for the per-base records `name p p+1 v`, p = s .. e-1.
 * The two files are independent streams, each read to its end; the checks and their order are those of the device reader
 * (csrc/bgrun.hip: rl_check, cornetto_bgrun_finish). */
void cli_runs_fail(const char *path, int kind, long long record, int a, int b)
{
    if (kind == 1 || kind == 2) {
        CLI_ERROR("%s: record %lld: a run-length depth record has 4 columns (name start end value). Had %d.", path, record, a);
    } else if (kind == 6) {
        CLI_ERROR("%s: record %lld: the first run of a contig should start at 0. Found %d", path, record, a);
    } else if (kind == 7) {
        CLI_ERROR("%s: record %lld: runs should follow each other without gap or overlap. Found end %d, then start %d "
                  "(`bedtools genomecov -bg` leaves out the zero-depth runs: use -bga)", path, record, a, b);
    } else if (kind == 8) {
        CLI_ERROR("%s: record %lld: a run should have end > start. Found %d to %d", path, record, a, b);
    } else if (kind == 9) {
        CLI_ERROR("%s: record %lld: negative depth value %d", path, record, a);
    } else {
        CLI_ERROR("%s: contig %lld is not the same in the two depth files (name, or length %d against %d)", path, record, a, b);
    }
    exit(EXIT_FAILURE);
}

/* %d of a WHOLE token, as the device readers convert it (csrc/bgtok.hpp parse_int): optional sign, digits, nothing else */
static int runs_int(const cli_str_t *t, int *v)
{
    size_t p = 0;
    int neg = 0;
    if (p < t->l && (t->s[p] == '-' || t->s[p] == '+')) neg = t->s[p++] == '-';
    if (p >= t->l) return 0;
    uint32_t x = 0;
    for (; p < t->l; ++p) {
        if (t->s[p] < '0' || t->s[p] > '9') return 0;
        x = x * 10u + (uint32_t)(t->s[p] - '0');
    }
    if (neg) x = 0u - x;
    memcpy(v, &x, sizeof(x));
    return 1;
}

typedef struct {
    int32_t n_ctg, cap_ctg;
    char **names;
    int32_t *lens;
    uint16_t *d;
    int64_t n_pos, cap_pos, n_clamped;
    double sum;
} runs_file_t;

static void runs_read(FILE *fp, const char *path, int file, runs_file_t *o)
{
    bgs_t s = {fp, (unsigned char *)cli_xmalloc(1 << 20), 0, 0, 0};
    cli_str_t name = {0, 0, 0}, tok = {0, 0, 0};
    memset(o, 0, sizeof(*o));
    int prev_end = 0;
    for (long long rec = 0;; ++rec) {
        int v[3] = {0, 0, 0}, conv = 1;
        if (!bgs_string(&s, &name)) break;
        while (conv < 4 && bgs_string(&s, &tok) && runs_int(&tok, &v[conv - 1])) ++conv;
        if (conv != 4) cli_runs_fail(path, 1 + file, rec, conv, 0);
        const int st = v[0], end = v[1];
        int depth = v[2];
        const int first = o->n_ctg == 0 || strcmp(name.s, o->names[o->n_ctg - 1]) != 0;
        if (first && st != 0) cli_runs_fail(path, 6, rec, st, 0);
        if (!first && st != prev_end) cli_runs_fail(path, 7, rec, prev_end, st);
        if (end <= st) cli_runs_fail(path, 8, rec, st, end);
        if (depth < 0) cli_runs_fail(path, 9, rec, depth, 0);
        if (first) {
            if (o->n_ctg == o->cap_ctg) {
                o->cap_ctg = o->cap_ctg ? o->cap_ctg * 2 : 256;
                o->names = (char **)cli_xrealloc(o->names, (size_t)o->cap_ctg * sizeof(char *));
                o->lens = (int32_t *)cli_xrealloc(o->lens, (size_t)o->cap_ctg * sizeof(int32_t));
            }
            o->names[o->n_ctg] = cli_xstrdup(name.s);
            o->lens[o->n_ctg++] = 0;
        }
        const int64_t len = (int64_t)end - st;
        if (depth > 65535) {
            depth = 65535;
            o->n_clamped += len;
        }
        if (o->n_pos + len > o->cap_pos) {
            while (o->n_pos + len > o->cap_pos) o->cap_pos = o->cap_pos ? o->cap_pos * 2 : 1 << 20;
            o->d = (uint16_t *)cli_xrealloc(o->d, (size_t)o->cap_pos * sizeof(uint16_t));
        }
        for (int64_t i = 0; i < len; ++i) o->d[o->n_pos + i] = (uint16_t)depth;
        o->n_pos += len;
        o->lens[o->n_ctg - 1] = end;       /* (a contig starts at 0 and has no gaps: its length is its last end) */
        o->sum += (double)depth * (double)len;
        prev_end = end;
    }
    free(s.buf);
    free(name.s);
    free(tok.s);
}

void cli_host_get_depths_runs(FILE *ft, FILE *fq, const char *path_t, const char *path_q, cli_host_cov_t *out)
{
    runs_file_t a, b;
    runs_read(ft, path_t, 0, &a);
    runs_read(fq, path_q, 1, &b);
    const int32_t n = a.n_ctg > b.n_ctg ? a.n_ctg : b.n_ctg;
    for (int32_t k = 0; k < n; ++k) {
        const int la = k < a.n_ctg ? a.lens[k] : 0, lb = k < b.n_ctg ? b.lens[k] : 0;
        if (k >= a.n_ctg || k >= b.n_ctg || la != lb || strcmp(a.names[k], b.names[k]) != 0) cli_runs_fail(path_t, 10, k, la, lb);
    }
    memset(out, 0, sizeof(*out));
    out->n_ctg = a.n_ctg;
    out->names = a.names;
    out->lens = a.lens;
    out->depth = a.d;
    out->mq = b.d;
    out->n_pos = a.n_pos;
    out->n_clamped = a.n_clamped + b.n_clamped;
    out->sum_depth = a.sum;
    out->sum_mq = b.sum;
    out->positions = (double)a.n_pos;
    if (a.n_ctg) {
        out->first = (int64_t *)cli_xmalloc(((size_t)a.n_ctg + 1) * sizeof(int64_t));
        out->first[0] = 0;
        for (int32_t k = 0; k < a.n_ctg; ++k) out->first[k + 1] = out->first[k] + a.lens[k];
    }
    for (int32_t k = 0; k < b.n_ctg; ++k) free(b.names[k]);
    free(b.names);
    free(b.lens);
}

/* ------------------------------------------------------------------------------------------------ get_depths, BAM
 * `--bam` (an extension, see boringbits_main.c and include/cornetto_accel.h for the rules): the file read sequentially through zlib (a
 * BGZF chain is a multi-member gzip file), one record at a time, the checks of the device reader in their order (csrc/bam.hpp). */
void cli_bam_fail(const char *path, int kind, long long record, int a, int b)
{
    if (kind == 1) {
        CLI_ERROR("%s: record %lld: block_size %d is below the 32 bytes of the fixed fields", path, record, a);
    } else if (kind == 2 && record < 0) {
        CLI_ERROR("%s: the file ends inside the BAM header", path);
    } else if (kind == 2) {
        CLI_ERROR("%s: record %lld: the file ends inside the record (%d bytes left, block_size %d)", path, record, a, b);
    } else if (kind == 3) {
        CLI_ERROR("%s: record %lld: the fixed fields ask for %d bytes, block_size is %d", path, record, a, b);
    } else if (kind == 4) {
        CLI_ERROR("%s: record %lld: refID %d is outside the %d contigs of the header", path, record, a, b);
    } else if (kind == 5) {
        CLI_ERROR("%s: record %lld: the CG array of %d operations runs past the record (%d bytes left)", path, record, a, b);
    } else if (kind == 6) {
        CLI_ERROR("%s: a BGZF block behind record %lld does not inflate to what its footer says", path, record);
    } else {
        CLI_ERROR("%s: not a BAM file", path);
    }
    cli_bgzf_out_flush();      /* (`seq --bam --bgzf`: the text of the records in front as a member; no end-of-file block) */
    exit(EXIT_FAILURE);
}

static uint32_t bam_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static int32_t bam_cap31(int64_t v) { return v > 0x7fffffffll ? 0x7fffffff : (int32_t)v; }

/* up to n bytes -> how many there were; a stream zlib cannot inflate: kind 6 */
static int64_t bam_read(gzFile f, const char *path, long long record, uint8_t *buf, int64_t n)
{
    int64_t got = 0;
    while (got < n) {
        const int want = n - got > (1 << 30) ? 1 << 30 : (int)(n - got);
        const int r = gzread(f, buf + got, (unsigned)want);
        if (r < 0) cli_bam_fail(path, 6, record, 0, 0);
        if (r == 0) break;
        got += r;
    }
    return got;
}

/* csrc/bam.hpp: cnb_find_cg */
static int bam_find_cg(const uint8_t *d, int64_t p, int64_t bs, const uint8_t **cig, int64_t *n_ops, int32_t *a, int32_t *b)
{
    while (bs - p >= 3) {
        const uint8_t t0 = d[p], t1 = d[p + 1], ty = d[p + 2];
        int64_t sz;
        p += 3;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (p < bs && d[p] != 0) ++p;
            if (p >= bs) return 0;
            sz = 1;
        } else if (ty == 'B') {
            if (bs - p < 5) return 0;
            const uint8_t sub = d[p];
            const int64_t cnt = (int64_t)bam_u32(d + p + 1);
            int64_t es;
            p += 5;
            if (sub == 'c' || sub == 'C') es = 1;
            else if (sub == 's' || sub == 'S') es = 2;
            else if (sub == 'i' || sub == 'I' || sub == 'f') es = 4;
            else return 0;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') {
                if (cnt * 4 > bs - p) {
                    *a = bam_cap31(cnt);
                    *b = (int32_t)(bs - p);
                    return -1;
                }
                *cig = d + p;
                *n_ops = cnt;
                return 1;
            }
            sz = cnt * es;
        } else return 0;
        if (sz > bs - p) return 0;
        p += sz;
    }
    return 0;
}

/* the file opened, its magic, header text and contig count read (a buffer of *cap bytes comes back with it) -> n_ref; the contigs follow */
static int32_t bam_host_open(const char *path, gzFile *fo, uint8_t **bufo, size_t *capo)
{
    gzFile f = gzopen(path, "rb");
    if (!f) {
        CLI_ERROR("Failed to open %s : No such file or directory.", path);
        exit(EXIT_FAILURE);
    }
    gzbuffer(f, 1 << 20);
    uint8_t w[8];
    int64_t got = bam_read(f, path, -1, w, 8);
    if (got > 0 && gzdirect(f)) cli_bam_fail(path, 7, -1, 0, 0);      /* (zlib hands bytes that are no gzip stream through as they are: no BAM, as on the device) */
    const size_t n_magic = got < 0 ? 0 : (got < 4 ? (size_t)got : 4);
    if (memcmp(w, "BAM\1", n_magic) != 0) cli_bam_fail(path, 7, -1, 0, 0);
    if (got < 8) cli_bam_fail(path, 2, -1, 0, -1);
    const int32_t l_text = (int32_t)bam_u32(w + 4);
    if (l_text < 0) cli_bam_fail(path, 7, -1, 0, 0);
    size_t cap = 1 << 16;
    uint8_t *buf = (uint8_t *)cli_xmalloc(cap);
    for (int64_t left = l_text; left > 0;) {
        const int64_t n = left < (int64_t)cap ? left : (int64_t)cap;
        if (bam_read(f, path, -1, buf, n) < n) cli_bam_fail(path, 2, -1, 0, -1);
        left -= n;
    }
    if (bam_read(f, path, -1, w, 4) < 4) cli_bam_fail(path, 2, -1, 0, -1);
    const int32_t n_ref = (int32_t)bam_u32(w);
    if (n_ref < 0) cli_bam_fail(path, 7, -1, 0, 0);
    *fo = f;
    *bufo = buf;
    *capo = cap;
    return n_ref;
}

/* the next contig of the header -> its length, its name (NUL-terminated) in *buf */
static int32_t bam_host_contig(gzFile f, const char *path, uint8_t **bufp, size_t *capp)
{
    uint8_t w[4];
    if (bam_read(f, path, -1, w, 4) < 4) cli_bam_fail(path, 2, -1, 0, -1);
    const int32_t l_name = (int32_t)bam_u32(w);
    if (l_name < 1) cli_bam_fail(path, 7, -1, 0, 0);
    if ((size_t)l_name + 4 > *capp) *bufp = (uint8_t *)cli_xrealloc(*bufp, *capp = (size_t)l_name + 4);
    if (bam_read(f, path, -1, *bufp, (int64_t)l_name + 4) < (int64_t)l_name + 4) cli_bam_fail(path, 2, -1, 0, -1);
    const int32_t l_ref = (int32_t)bam_u32(*bufp + l_name);
    if (l_ref < 0) cli_bam_fail(path, 7, -1, 0, 0);
    (*bufp)[l_name - 1] = 0;
    return l_ref;
}

/* record `rec` of the file into *buf, checks 1 to 4 passed -> its block_size, or -1: the file ends in front of it */
static int32_t bam_host_record(gzFile f, const char *path, long long rec, int32_t n_ref, uint8_t **bufp, size_t *capp)
{
    uint8_t w[4];
    uint8_t *buf = *bufp;
    size_t cap = *capp;
    int64_t got = bam_read(f, path, rec, w, 4);
    if (got == 0) return -1;
    if (got < 4) cli_bam_fail(path, 2, rec, (int)got, -1);
    const int32_t bs = (int32_t)bam_u32(w);
    if (bs < 32) cli_bam_fail(path, 1, rec, bs, 0);
    got = 0;
    for (int64_t n = 0; got == n && n < bs;) {      /* (the buffer grows with the bytes that are there, not with what block_size says) */
        if ((size_t)bs > cap && (size_t)n == cap) buf = (uint8_t *)cli_xrealloc(buf, cap = cap * 2 < (size_t)bs ? cap * 2 : (size_t)bs);
        n = (int64_t)cap < bs ? (int64_t)cap : bs;
        got += bam_read(f, path, rec, buf + got, n - got);
    }
    *bufp = buf;
    *capp = cap;
    if (got < bs) cli_bam_fail(path, 2, rec, bam_cap31(got + 4), bs);
    const int32_t ref_id = (int32_t)bam_u32(buf);
    const int64_t l_read_name = buf[8], n_cigar = (int64_t)buf[12] | ((int64_t)buf[13] << 8), l_seq = (int64_t)bam_u32(buf + 16);
    const int64_t fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    if (fixed > bs) cli_bam_fail(path, 3, rec, bam_cap31(fixed), bs);
    if (ref_id < -1 || ref_id >= n_ref) cli_bam_fail(path, 4, rec, ref_id, n_ref);
    return bs;
}

void cli_host_get_depths_bam(const char *path, int min_mapq, cli_host_cov_t *out)
{
    gzFile f = NULL;
    uint8_t *buf = NULL;
    size_t cap = 0;
    const int32_t n_ref = bam_host_open(path, &f, &buf, &cap);
    /* every contig of the header, in its order; `all_first` places it in the arrays (a contig without positions has no line in a per-base
     * bedgraph: it is not a contig of the result) */
    int32_t *all_len = (int32_t *)cli_xmalloc(((size_t)n_ref + 1) * sizeof(int32_t));
    int64_t *all_first = (int64_t *)cli_xmalloc(((size_t)n_ref + 1) * sizeof(int64_t));
    memset(out, 0, sizeof(*out));
    out->names = (char **)cli_xmalloc(((size_t)n_ref + 1) * sizeof(char *));
    out->lens = (int32_t *)cli_xmalloc(((size_t)n_ref + 1) * sizeof(int32_t));
    out->first = (int64_t *)cli_xmalloc(((size_t)n_ref + 2) * sizeof(int64_t));
    out->first[0] = 0;
    int64_t n_pos = 0;
    for (int32_t i = 0; i < n_ref; ++i) {
        const int32_t l_ref = bam_host_contig(f, path, &buf, &cap);
        all_len[i] = l_ref;
        all_first[i] = n_pos;
        if (l_ref > 0) {
            out->names[out->n_ctg] = cli_xstrdup((const char *)buf);
            out->lens[out->n_ctg] = l_ref;
            out->first[++out->n_ctg] = n_pos + l_ref;
        }
        n_pos += l_ref;
    }
    int32_t *diff[2];
    for (int q = 0; q < 2; ++q) {
        diff[q] = (int32_t *)calloc((size_t)n_pos + 1, sizeof(int32_t));
        if (!diff[q]) {
            CLI_ERROR("cannot allocate the depth arrays of %lld positions", (long long)n_pos);
            exit(EXIT_FAILURE);
        }
    }
    for (long long rec = 0;; ++rec) {
        const int32_t bs = bam_host_record(f, path, rec, n_ref, &buf, &cap);
        if (bs < 0) break;
        const int32_t ref_id = (int32_t)bam_u32(buf), pos = (int32_t)bam_u32(buf + 4);
        const int64_t l_read_name = buf[8], n_cigar = (int64_t)buf[12] | ((int64_t)buf[13] << 8), l_seq = (int64_t)bam_u32(buf + 16);
        const int mapq = buf[9], flag = (int)buf[14] | ((int)buf[15] << 8);
        const int64_t fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
        if (ref_id < 0 || (flag & 0x704) != 0) continue;
        const uint8_t *cig = buf + 32 + l_read_name;
        int64_t n_ops = n_cigar;
        if (n_cigar == 2) {
            const uint32_t op0 = bam_u32(cig), op1 = bam_u32(cig + 4);
            int32_t a = 0, b = 0;
            if ((op0 & 15u) == 4u && (int64_t)(op0 >> 4) == l_seq && (op1 & 15u) == 3u && bam_find_cg(buf, fixed, bs, &cig, &n_ops, &a, &b) < 0)
                cli_bam_fail(path, 5, rec, a, b);
        }
        const int64_t len = all_len[ref_id], base = all_first[ref_id];
        int64_t at = pos;
        for (int64_t i = 0; i < n_ops; ++i) {
            const uint32_t op = bam_u32(cig + 4 * i), k = op & 15u;
            const int64_t n = op >> 4;
            if (k == 0 || k == 7 || k == 8) {
                int64_t s = at, e = at + n;
                s = s < 0 ? 0 : (s > len ? len : s);
                e = e < 0 ? 0 : (e > len ? len : e);
                if (s < e) {
                    diff[0][base + s]++;
                    diff[0][base + e]--;
                    if (mapq >= min_mapq) {
                        diff[1][base + s]++;
                        diff[1][base + e]--;
                    }
                }
                at += n;
            } else if (k == 2 || k == 3) {
                at += n;
            }
        }
    }
    gzclose(f);
    free(buf);
    free(all_len);
    free(all_first);
    out->depth = (uint16_t *)cli_xmalloc(((size_t)n_pos + 1) * sizeof(uint16_t));
    out->mq = (uint16_t *)cli_xmalloc(((size_t)n_pos + 1) * sizeof(uint16_t));
    for (int q = 0; q < 2; ++q) {
        uint16_t *dst = q ? out->mq : out->depth;
        double sum = 0.0;
        int64_t run = 0;
        for (int64_t i = 0; i < n_pos; ++i) {
            run += diff[q][i];
            int64_t v = run;
            if (v > 65535) {
                v = 65535;
                out->n_clamped++;
            }
            dst[i] = (uint16_t)v;
            sum += (double)v;
        }
        if (q) out->sum_mq = sum;
        else out->sum_depth = sum;
        free(diff[q]);
    }
    out->n_pos = n_pos;
    out->positions = (double)n_pos;
}

/* ------------------------------------------------------------------------------------------------ seq --bam
 * The FASTQ text of a BAM (an extension, see fasta_cmds.c and include/cornetto_accel.h for the rules): the file read sequentially through
 * zlib, one record at a time, the checks and rules of the device reader in their order (csrc/bamfq.hpp). */
/* csrc/bamfq.hpp: cnq_find_dx */
static int bam_find_dx(const uint8_t *d, int64_t p, int64_t bs, int64_t *val)
{
    while (bs - p >= 3) {
        const uint8_t t0 = d[p], t1 = d[p + 1], ty = d[p + 2];
        int64_t sz;
        p += 3;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (p < bs && d[p] != 0) ++p;
            if (p >= bs) return 0;
            sz = 1;
        } else if (ty == 'B') {
            if (bs - p < 5) return 0;
            const uint8_t sub = d[p];
            const int64_t cnt = (int64_t)bam_u32(d + p + 1);
            int64_t es;
            p += 5;
            if (sub == 'c' || sub == 'C') es = 1;
            else if (sub == 's' || sub == 'S') es = 2;
            else if (sub == 'i' || sub == 'I' || sub == 'f') es = 4;
            else return 0;
            sz = cnt * es;
        } else return 0;
        if (sz > bs - p) return 0;
        if (t0 == 'd' && t1 == 'x' && (ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I')) {
            const uint32_t lo16 = (uint32_t)d[p] | (sz > 1 ? (uint32_t)d[p + 1] << 8 : 0u);
            if (ty == 'c') *val = (int8_t)d[p];
            else if (ty == 'C') *val = d[p];
            else if (ty == 's') *val = (int16_t)lo16;
            else if (ty == 'S') *val = (int64_t)lo16;
            else if (ty == 'i') *val = (int32_t)bam_u32(d + p);
            else *val = (int64_t)bam_u32(d + p);
            return 1;
        }
        p += sz;
    }
    return 0;
}

void cli_host_bam_fastq(const char *path, int min_len, int duplex, int64_t skip_records, uint64_t stats[4])
{
    static const char fwd[] = "=ACMGRSVTWYHKDBN", rev[] = "=TGKCYSBAWRDMHVN";
    gzFile f = NULL;
    uint8_t *buf = NULL;
    size_t cap = 0, cap_line = 0;
    char *line = NULL;
    const int32_t n_ref = bam_host_open(path, &f, &buf, &cap);
    for (int32_t i = 0; i < n_ref; ++i) (void)bam_host_contig(f, path, &buf, &cap);
    for (long long rec = 0;; ++rec) {
        const int32_t bs = bam_host_record(f, path, rec, n_ref, &buf, &cap);
        if (bs < 0) break;
        if (rec < skip_records) continue;      /* (printed and counted by the caller already) */
        const int64_t l_read_name = buf[8], n_cigar = (int64_t)buf[12] | ((int64_t)buf[13] << 8), l_seq = (int64_t)bam_u32(buf + 16);
        const int flag = (int)buf[14] | ((int)buf[15] << 8);
        if (flag & 0x900) continue;
        stats[0]++;
        stats[1] += (uint64_t)l_seq;
        if (l_seq < min_len) continue;
        if (duplex) {
            int64_t v = 0;
            if (!bam_find_dx(buf, 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq, bs, &v) || v != 1) continue;
        }
        stats[2]++;
        stats[3] += (uint64_t)l_seq;
        const int64_t name_len = l_read_name ? l_read_name - 1 : 0;
        const size_t need = (size_t)(name_len + 2 * l_seq + 6);
        if (need > cap_line) line = (char *)cli_xrealloc(line, cap_line = need * 2);
        const uint8_t *seq = buf + 32 + l_read_name + 4 * n_cigar, *qual = seq + (l_seq + 1) / 2;
        const int rv = (flag & 0x10) != 0, no_qual = l_seq > 0 && qual[0] == 0xFF;
        char *o = line;
        *o++ = '@';
        memcpy(o, buf + 32, (size_t)name_len);
        o += name_len;
        *o++ = '\n';
        for (int64_t i = 0; i < l_seq; ++i) {
            const int64_t j = rv ? l_seq - 1 - i : i;
            const int nib = (j & 1) ? (seq[j >> 1] & 15) : (seq[j >> 1] >> 4);
            *o++ = rv ? rev[nib] : fwd[nib];
        }
        *o++ = '\n';
        *o++ = '+';
        *o++ = '\n';
        for (int64_t i = 0; i < l_seq; ++i) {
            const int q = qual[rv ? l_seq - 1 - i : i];
            *o++ = no_qual ? '"' : (char)((q > 93 ? 93 : q) + 33);
        }
        *o++ = '\n';
        if (!cli_qmean_pass(o - 1 - l_seq, (size_t)l_seq, l_seq)) continue;      /* -q: decided on the quality line as it is printed */
        cli_qmean_count(l_seq);
        if (cli_bgzf_out_active()) cli_bgzf_out_text(line, need);
        else fwrite(line, 1, need, stdout);
    }
    gzclose(f);
    free(buf);
    free(line);
}

void cli_host_cov_free(cli_host_cov_t *c)
{
    for (int32_t i = 0; i < c->n_ctg; ++i) free(c->names[i]);
    free(c->names);
    free(c->lens);
    free(c->first);
    free(c->depth);
    free(c->mq);
    memset(c, 0, sizeof(*c));
}

/* ------------------------------------------------------------------------------------------------ get_regs + selection
 * src/boringbits_main.c:322-378 and the predicates of :425-445 / :463-481.  The window sums slide (what leaves, what
 * enters) in 32-bit unsigned arithmetic: the same value as the reference's `int` sums modulo 2^32. */
void cli_host_cov_select(const cli_host_cov_t *c, int w, int inc, int32_t lo, int32_t hi, float low_mq, int32_t edge_len, int32_t min_ctg_len, int boring,
                         cornetto_regrec_t **recs, int64_t *n_recs)
{
    cornetto_regrec_t *o = NULL;
    int64_t n = 0, cap = 0;
    for (int32_t ci = 0; ci < c->n_ctg; ++ci) {
        const int32_t len = c->lens[ci];
        if (boring ? !(len > min_ctg_len) : len < min_ctg_len) continue;                /* :467 / :428 */
        const uint16_t *dp = c->depth + c->first[ci], *mq = c->mq + c->first[ci];
        int32_t n_reg = (len - w + inc - 1) / inc + 1;                                 /* :338 */
        if (n_reg < 1) n_reg = 1;                                                      /* :339 */
        uint32_t sd = 0, sq = 0;
        int64_t a = 0, b = 0; /* the sums hold [a, b) */
        for (int32_t j = 0; j < n_reg; ++j) {
            const int64_t st = (int64_t)j * inc;
            int64_t end = st + w;
            if (end > len) end = len;                                                  /* :349-351 */
            /* (st < end: the caller has run the asserts of :353 / :368 over every contig — cornetto_regs_assert) */
            if (st >= b) {
                sd = sq = 0;
                a = b = st;
            }
            for (; a < st; ++a) {
                sd -= dp[a];
                sq -= mq[a];
            }
            for (; b < end; ++b) {
                sd += dp[b];
                sq += mq[b];
            }
            const int32_t depth = (int32_t)sd / (int32_t)(end - st), mqd = (int32_t)sq / (int32_t)(end - st);   /* :360-361 */
            const int fun = depth < lo || depth > hi || (mqd / (double)depth) < low_mq;                         /* :439 */
            const int sel = boring ? (st > edge_len && end < len - edge_len && !fun) : fun;                      /* :473-474 */
            if (!sel) continue;
            if (n == cap) {
                cap = cap ? cap * 2 : 4096;
                o = (cornetto_regrec_t *)cli_xrealloc(o, (size_t)cap * sizeof(*o));
            }
            o[n].ctg = ci;
            o[n].st = (int32_t)st;
            o[n].end = (int32_t)end;
            o[n].depth = depth;
            o[n].mq_depth = mqd;
            ++n;
        }
    }
    *recs = o;
    *n_recs = n;
}

/* the first three steps of scripts/create-cornetto.sh (:41-47) on the selected windows: `bedtools merge -d dist` of rows
 * that are already ordered (a row opens a new interval iff it starts more than dist behind the furthest end so far),
 * then the rows of at least min_len */
void cli_host_merge_windows(const cornetto_regrec_t *recs, int64_t n_recs, int32_t dist, int32_t min_len, cornetto_ivl_t **ivls, int64_t *n_ivls)
{
    cornetto_ivl_t *o = (cornetto_ivl_t *)cli_xmalloc(((size_t)n_recs + 1) * sizeof(*o));
    int64_t n = 0;
    for (int64_t i = 0; i < n_recs; ++i) {
        if (n > 0 && o[n - 1].ctg == recs[i].ctg && (int64_t)recs[i].st <= (int64_t)o[n - 1].finish + dist) {
            if (recs[i].end > o[n - 1].finish) o[n - 1].finish = recs[i].end;
        } else {
            if (n > 0 && o[n - 1].finish - o[n - 1].start < min_len) --n;
            o[n].ctg = recs[i].ctg;
            o[n].start = recs[i].st;
            o[n].finish = recs[i].end;
            ++n;
        }
    }
    if (n > 0 && o[n - 1].finish - o[n - 1].start < min_len) --n;
    *ivls = o;
    *n_ivls = n;
}

/* ------------------------------------------------------------------------------------------------ the haplotype stage
 * scripts/create-hapnetto.sh:40-67 step by step, sequential: per haplotype a loop over its queries (:48-51: the rows of one query sorted by
 * target and start, merge -d merge_dist), the gaps of every contig (:55), the corners of every block (:58), sort + merge (:61); then the
 * haplotypes together (:67).  No library call. */
static int hap_by_query(const void *a_, const void *b_)
{
    const cornetto_hap_row_t *a = (const cornetto_hap_row_t *)a_, *b = (const cornetto_hap_row_t *)b_;
    if (a->query != b->query) return a->query < b->query ? -1 : 1;
    if (a->ctg != b->ctg) return a->ctg < b->ctg ? -1 : 1;
    return a->start < b->start ? -1 : a->start > b->start;
}

static int hap_by_pos(const void *a_, const void *b_)
{
    const cornetto_ivl_t *a = (const cornetto_ivl_t *)a_, *b = (const cornetto_ivl_t *)b_;
    if (a->ctg != b->ctg) return a->ctg < b->ctg ? -1 : 1;
    return a->start < b->start ? -1 : a->start > b->start;
}

/* bedtools sort | bedtools merge -d dist, in place -> the number of rows left */
static int64_t hap_sort_merge(cornetto_ivl_t *v, int64_t n, int32_t dist)
{
    qsort(v, (size_t)n, sizeof(*v), hap_by_pos);
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (m > 0 && v[m - 1].ctg == v[i].ctg && (int64_t)v[i].start <= (int64_t)v[m - 1].finish + dist) {
            if (v[i].finish > v[m - 1].finish) v[m - 1].finish = v[i].finish;
        } else {
            v[m++] = v[i];
        }
    }
    return m;
}

typedef struct {
    cornetto_ivl_t *v;
    int64_t n, cap;
} hap_list_t;

static void hap_push(hap_list_t *l, int32_t ctg, int64_t start, int64_t finish)
{
    if (l->n == l->cap) {
        l->cap = l->cap ? l->cap * 2 : 1024;
        l->v = (cornetto_ivl_t *)cli_xrealloc(l->v, (size_t)l->cap * sizeof(*l->v));
    }
    l->v[l->n].ctg = ctg;
    l->v[l->n].start = (int32_t)start;
    l->v[l->n].finish = (int32_t)(finish < INT32_MAX ? finish : INT32_MAX);
    ++l->n;
}

void cli_host_hap_fun(const int32_t *ctg_len, int32_t n_ctg, const cornetto_hap_row_t *rows, const int64_t *n_rows, int32_t n_hap, int32_t merge_dist, int32_t flank,
                      cornetto_ivl_t **fun, int64_t *n_fun)
{
    hap_list_t all = {NULL, 0, 0};
    int64_t at = 0;
    for (int32_t k = 0; k < n_hap; at += n_rows[k], ++k) {
        const int64_t n = n_rows[k];
        cornetto_hap_row_t *r = (cornetto_hap_row_t *)cli_xmalloc(((size_t)n + 1) * sizeof(*r));
        memcpy(r, rows + at, (size_t)n * sizeof(*r));
        qsort(r, (size_t)n, sizeof(*r), hap_by_query);
        /* :48-51 every query on its own: its rows as BED intervals on their targets, sort, merge -d */
        hap_list_t blocks = {NULL, 0, 0};
        for (int64_t i = 0; i < n;) {
            int64_t e = i;
            while (e < n && r[e].query == r[i].query) ++e;
            cornetto_ivl_t *q = (cornetto_ivl_t *)cli_xmalloc((size_t)(e - i) * sizeof(*q));
            for (int64_t j = i; j < e; ++j) {
                q[j - i].ctg = r[j].ctg;
                q[j - i].start = r[j].start;
                q[j - i].finish = r[j].finish;
            }
            const int64_t m = hap_sort_merge(q, e - i, merge_dist);
            for (int64_t j = 0; j < m; ++j) hap_push(&blocks, q[j].ctg, q[j].start, q[j].finish);
            free(q);
            i = e;
        }
        free(r);
        /* :55 the gaps: every contig minus the blocks on it */
        hap_list_t tmp2 = {NULL, 0, 0};
        cornetto_ivl_t *b = (cornetto_ivl_t *)cli_xmalloc(((size_t)blocks.n + 1) * sizeof(*b));
        memcpy(b, blocks.v, (size_t)blocks.n * sizeof(*b));
        qsort(b, (size_t)blocks.n, sizeof(*b), hap_by_pos);
        int64_t j = 0;
        for (int32_t c = 0; c < n_ctg; ++c) {
            int64_t pos = 0;
            const int64_t len = ctg_len[c];
            for (; j < blocks.n && b[j].ctg == c; ++j) {
                const int64_t s = b[j].start < len ? b[j].start : len, e = b[j].finish < len ? b[j].finish : len;
                if (s > pos) hap_push(&tmp2, c, pos, s);
                if (e > pos) pos = e;
            }
            if (pos < len) hap_push(&tmp2, c, pos, len);
        }
        free(b);
        /* :58 the corners of every block, as the awk prints them (the right one is not clamped to the contig) */
        for (int64_t i = 0; i < blocks.n; ++i) {
            if (blocks.v[i].start >= flank) hap_push(&tmp2, blocks.v[i].ctg, (int64_t)blocks.v[i].start - flank, (int64_t)blocks.v[i].start + flank);
            if (blocks.v[i].finish >= flank) hap_push(&tmp2, blocks.v[i].ctg, (int64_t)blocks.v[i].finish - flank, (int64_t)blocks.v[i].finish + flank);
        }
        free(blocks.v);
        /* :61 */
        const int64_t m = hap_sort_merge(tmp2.v, tmp2.n, 0);
        for (int64_t i = 0; i < m; ++i) hap_push(&all, tmp2.v[i].ctg, tmp2.v[i].start, tmp2.v[i].finish);
        free(tmp2.v);
    }
    /* :67 */
    if (!all.v) all.v = (cornetto_ivl_t *)cli_xmalloc(sizeof(*all.v));
    *n_fun = hap_sort_merge(all.v, all.n, 0);
    *fun = all.v;
}

/* ------------------------------------------------------------------------------------------------ telostats --breaks
 * test/realtest.sh:65-69 on one record: sdust, telofind, then src/telomere_breaks.c:95-148 as the rule on intervals of
 * csrc/telobreaks_ivl.hip — what sdust prints is sorted with every start beyond the previous finish (src/sdust/sdust.c:88-102), so the
 * intervals are the runs of the reference's bitset.  Sequential: one binary search per run of at least 24 bases. */
int cli_host_telo_breaks(const uint8_t *seq, int64_t len, const char *motif, int T, int W, int32_t ctg, cornetto_ivl_t **rows, int64_t *n_rows, int64_t *cap_rows)
{
    cornetto_ivl_t *sd = NULL;
    cornetto_hit_t *hits = NULL;
    int64_t n_sd = 0, cap_sd = 0, n_hits = 0, cap_hits = 0;
    if (cli_host_sdust(seq, len, T, W, 0, &sd, &n_sd, &cap_sd) != 0) return -1;
    cli_host_telofind(seq, len, motif, 0, &hits, &n_hits, &cap_hits);
    uint8_t *mark = (uint8_t *)cli_xmalloc((size_t)n_sd + 1);
    memset(mark, 0, (size_t)n_sd + 1);
    for (int64_t i = 1; i < n_sd; ++i)
        if (sd[i].start <= sd[i - 1].finish) {
            CLI_ERROR("sdust intervals %d-%d and %d-%d of one record touch or are out of order", sd[i - 1].start, sd[i - 1].finish, sd[i].start, sd[i].finish);
            exit(EXIT_FAILURE);
        }
    for (int64_t i = 0; i < n_hits; ++i) {
        if (hits[i].end - hits[i].start < 24) continue;                               /* MIN_TEL, :10,:98 */
        const int64_t a = hits[i].start - 100 < 0 ? 0 : hits[i].start - 100, b = (int64_t)hits[i].end + 100 > len ? len : hits[i].end + 100;   /* :102-103 */
        int64_t lo = 0, hi = n_sd;                                                    /* lo = intervals that start at or before a */
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (sd[mid].start <= a) lo = mid + 1;
            else hi = mid;
        }
        if (lo > 0 && (sd[lo - 1].finish > len ? len : sd[lo - 1].finish) >= b) mark[lo - 1] = 1;
    }
    for (int64_t i = 0; i < n_sd; ++i) {
        if (!mark[i]) continue;
        if (*n_rows == *cap_rows) {
            *cap_rows = *cap_rows ? *cap_rows * 2 : 64;
            *rows = (cornetto_ivl_t *)cli_xrealloc(*rows, (size_t)*cap_rows * sizeof(**rows));
        }
        (*rows)[*n_rows].ctg = ctg;
        (*rows)[*n_rows].start = sd[i].start - 1 < 0 ? 0 : sd[i].start - 1;           /* :139-142 */
        (*rows)[*n_rows].finish = (int32_t)((sd[i].finish > len ? len : sd[i].finish) - 1);
        ++*n_rows;
    }
    free(mark);
    free(sd);
    free(hits);
    return 0;
}

/* ------------------------------------------------------------------------------------------------ telobreaks
 * src/telomere_breaks.c:79-148: one bit per base for the low-complexity intervals, a second bit set for the runs of it
 * that hold a telomere row with its 100-base flanks; the runs of the second set are the output. */
static inline int bit_at(const uint64_t *w, int64_t i) { return (int)(w[i >> 6] >> (i & 63)) & 1; }

int cli_host_telobreaks(const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *sd, int64_t n_sd, const cornetto_telrow_t *tel, int64_t n_tel,
                        cornetto_ivl_t **out, int64_t *n_out)
{
    uint64_t **low = (uint64_t **)cli_xmalloc(((size_t)n_ctg + 1) * sizeof(*low)), **fin = (uint64_t **)cli_xmalloc(((size_t)n_ctg + 1) * sizeof(*fin));
    for (int32_t c = 0; c < n_ctg; ++c) {
        low[c] = (uint64_t *)calloc((size_t)(ctg_len[c] / 64 + 2), 8);
        fin[c] = (uint64_t *)calloc((size_t)(ctg_len[c] / 64 + 2), 8);
        if (!low[c] || !fin[c]) {
            CLI_ERROR("%s", "out of memory");
            exit(EXIT_FAILURE);
        }
    }
    int rc = 0;
    for (int64_t i = 0; i < n_sd && !rc; ++i) {                                       /* :79-90 */
        if (sd[i].ctg < 0 || sd[i].ctg >= n_ctg) continue;
        /* (beyond the contig's end: sdust's own intervals at a contig's end reach there; the reference sets those bits and never reads them) */
        const int64_t fin_i = sd[i].finish > ctg_len[sd[i].ctg] ? ctg_len[sd[i].ctg] : sd[i].finish;
        if (sd[i].start < 0) rc = -1;
        else if (sd[i].start < fin_i) bits_set(low[sd[i].ctg], sd[i].start, fin_i);
    }
    for (int64_t i = 0; i < n_tel && !rc; ++i) {                                      /* :95-128 */
        if (tel[i].matched < 24 || tel[i].ctg < 0 || tel[i].ctg >= n_ctg) continue;   /* MIN_TEL, :10,:98 */
        const int64_t len = ctg_len[tel[i].ctg];
        if (tel[i].start < 0 || tel[i].end > len || tel[i].start >= tel[i].end) {
            rc = -1;
            break;
        }
        const uint64_t *b = low[tel[i].ctg];
        const int64_t a0 = tel[i].start - 100 < 0 ? 0 : tel[i].start - 100, a1 = tel[i].end + 100 > len ? len : tel[i].end + 100;   /* :102-103 */
        if (bits_in(b, a0, a1) != a1 - a0) continue;
        int64_t s = tel[i].start, e = tel[i].end;                                     /* :114-121 */
        while (s > 0 && bit_at(b, s - 1)) --s;
        while (e < len && bit_at(b, e)) ++e;
        bits_set(fin[tel[i].ctg], s, e);
    }
    cornetto_ivl_t *o = NULL;
    int64_t n = 0, cap = 0;
    for (int32_t c = 0; c < n_ctg && !rc; ++c) {                                      /* :133-148 */
        const int64_t len = ctg_len[c];
        for (int64_t i = 0; i < len; ++i) {
            if (!fin[c][i >> 6]) {
                i |= 63;
                continue;
            }
            if (!bit_at(fin[c], i)) continue;
            int64_t e = i;
            while (e < len && bit_at(fin[c], e)) ++e;
            if (n == cap) {
                cap = cap ? cap * 2 : 256;
                o = (cornetto_ivl_t *)cli_xrealloc(o, (size_t)cap * sizeof(*o));
            }
            o[n].ctg = c;
            o[n].start = (int32_t)(i - 1 < 0 ? 0 : i - 1);                             /* :139-141 */
            o[n].finish = (int32_t)(e - 1);
            ++n;
            i = e;
        }
    }
    for (int32_t c = 0; c < n_ctg; ++c) {
        free(low[c]);
        free(fin[c]);
    }
    free(low);
    free(fin);
    if (rc) {
        free(o);
        o = NULL;
        n = 0;
    }
    *out = o;
    *n_out = n;
    return rc;
}
