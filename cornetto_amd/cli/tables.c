/* tables.c — the small text tables the assembly sub-commands share: a string -> index map, the PAF line of src/pafrec.c:43-98 (fixasm,
 * asmstats), the four PAF columns of scripts/create-hapnetto.sh:44,50 (noboringbits --hap), the telomere BED of src/telocontigs.c:59-108 / src/asmstats.c:230-290 (telocontigs, asmstats) and the natural name order of
 * src/misc.c:139-171 (asmstats). */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "cli.h"

FILE *cli_fopen_chk(const char *path, const char *mode)
{
    FILE *f = fopen(path, mode);
    if (!f) {
        CLI_ERROR("Could not to open file %s: %s", path, strerror(errno)); /* F_CHK, src/error.h:114-119: its words */
        exit(EXIT_FAILURE);
    }
    return f;
}

/* ---------------------------------------------------------------- a string -> index map */
static uint64_t map_hash(const char *s, size_t n)
{
    uint64_t h = 1469598103934665603ULL;
    for (size_t i = 0; i < n; ++i) h = (h ^ (uint8_t)s[i]) * 1099511628211ULL;
    return h;
}

int32_t cli_map_get(const cli_map_t *m, const char *s, size_t n)
{
    if (!m->cap) return -1;
    for (size_t i = map_hash(s, n) & (m->cap - 1);; i = (i + 1) & (m->cap - 1)) {
        const int32_t v = m->slot[i];
        if (!v) return -1;
        if ((size_t)m->klen[v - 1] == n && !memcmp(m->keys[v - 1], s, n)) return v - 1;
    }
}

int32_t cli_map_put(cli_map_t *m, const char *s, size_t n, int *added)
{
    *added = 0;
    const int32_t have = cli_map_get(m, s, n);
    if (have >= 0) return have;
    if ((m->n + 1) * 2 > m->cap) {
        const size_t cap = m->cap ? m->cap * 2 : 1024;
        int32_t *slot = (int32_t *)calloc(cap, sizeof(int32_t));
        if (!slot) { CLI_ERROR("Failed to allocate memory: %s", strerror(errno)); exit(EXIT_FAILURE); }
        for (size_t k = 0; k < m->n; ++k) {
            size_t i = map_hash(m->keys[k], (size_t)m->klen[k]) & (cap - 1);
            while (slot[i]) i = (i + 1) & (cap - 1);
            slot[i] = (int32_t)k + 1;
        }
        free(m->slot);
        m->slot = slot;
        m->cap = cap;
    }
    if (m->n == m->kcap) {
        m->kcap = m->kcap ? m->kcap * 2 : 256;
        m->keys = (char **)cli_xrealloc(m->keys, m->kcap * sizeof(char *));
        m->klen = (int32_t *)cli_xrealloc(m->klen, m->kcap * sizeof(int32_t));
    }
    char *k = (char *)cli_xmalloc(n + 1);
    memcpy(k, s, n);
    k[n] = 0;
    m->keys[m->n] = k;
    m->klen[m->n] = (int32_t)n;
    size_t i = map_hash(s, n) & (m->cap - 1);
    while (m->slot[i]) i = (i + 1) & (m->cap - 1);
    m->slot[i] = (int32_t)m->n + 1;
    *added = 1;
    return (int32_t)m->n++;
}

void cli_map_free(cli_map_t *m)
{
    for (size_t k = 0; k < m->n; ++k) free(m->keys[k]);
    free(m->keys);
    free(m->klen);
    free(m->slot);
    memset(m, 0, sizeof(*m));
}

/* ---------------------------------------------------------------- the PAF (src/pafrec.c:43-98) */
static int32_t paf_atoi(const char *s) { return (int32_t)strtol(s, NULL, 10); }   /* glibc's atoi() */

static char *paf_field(char **save)
{
    char *p = strtok_r(NULL, "\t\r\n", save);
    if (!p) {
        CLI_ERROR("%s", "Malformed PAF record. Exiting.");
        exit(EXIT_FAILURE);
    }
    return p;
}

void cli_paf_parse(char *line, cli_paf_t *r)
{
    char *save = NULL;
    char *p = strtok_r(line, "\t\r\n", &save);
    if (!p) {
        CLI_ERROR("%s", "Malformed PAF record. Exiting.");
        exit(EXIT_FAILURE);
    }
    r->rid = p;
    r->qlen = paf_atoi(paf_field(&save));
    r->qs = paf_atoi(paf_field(&save));
    r->qe = paf_atoi(paf_field(&save));
    r->strand = strcmp(paf_field(&save), "+") == 0 ? 0 : 1;
    r->tid = paf_field(&save);
    r->tlen = paf_atoi(paf_field(&save));
    r->ts = paf_atoi(paf_field(&save));
    r->te = paf_atoi(paf_field(&save));
    r->match = paf_atoi(paf_field(&save));
    r->block = paf_atoi(paf_field(&save));
    r->mapq = (uint8_t)paf_atoi(paf_field(&save));
    r->tp = 'P';
    while ((p = strtok_r(NULL, "\t\r\n", &save))) {
        if (!strcmp(p, "tp:A:P")) r->tp = 'P';
        else if (!strcmp(p, "tp:A:S")) r->tp = 'S';
    }
}

/* ---------------------------------------------------------------- the PAF columns of the haplotype stage (scripts/create-hapnetto.sh:44,50)
 * The script cuts fields 1-10 and uses 1, 6, 8 and 9: the first nine tab-separated fields must be there, the rest of the line (cg:Z: tags of
 * megabytes) is not looked at.  getline() takes lines of any length. */
static int32_t hap_coord(const char *s, const char *e, const char *path, long long line_no, int col)
{
    long long v = 0;
    const char *p = s;
    const int neg = p < e && *p == '-';
    if (neg) ++p;
    if (p == e) v = -1;
    for (; p < e && v >= 0; ++p) {
        if (*p < '0' || *p > '9') v = -1;
        else if ((v = v * 10 + (*p - '0')) > 0x7fffffffLL) v = -2;
    }
    if (v == -1) {
        CLI_ERROR("%s: line %lld: column %d is not a number", path, line_no, col);
        exit(EXIT_FAILURE);
    }
    if (v == -2 || neg) {
        CLI_ERROR("%s: line %lld: column %d is negative or beyond 2^31-1", path, line_no, col);
        exit(EXIT_FAILURE);
    }
    return (int32_t)v;
}

int64_t cli_hap_paf_load(const char *path, cli_name_find_fn find_ctg, void *arg, cornetto_hap_row_t **rows, int64_t *n, int64_t *cap, int64_t *n_dropped)
{
    FILE *fp = fopen(path, "r");
    if (!fp) {
        CLI_ERROR("Failed to open %s : No such file or directory.", path);
        exit(EXIT_FAILURE);
    }
    cli_map_t queries;
    memset(&queries, 0, sizeof(queries));
    char *line = NULL;
    size_t lcap = 0;
    ssize_t got;
    long long line_no = 0;
    int64_t n_used = 0;
    *n_dropped = 0;
    while ((got = getline(&line, &lcap, fp)) != -1) {
        ++line_no;
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) --got;
        if (got == 0) continue; /* (an empty line: neither cut nor awk makes a row of it) */
        const char *fs[9], *fe[9];
        int nf = 0;
        const char *p = line, *end = line + got;
        while (nf < 9) {
            const char *t = (const char *)memchr(p, '\t', (size_t)(end - p));
            fs[nf] = p;
            fe[nf] = t ? t : end;
            ++nf;
            if (!t) break;
            p = t + 1;
        }
        if (nf < 9) {
            CLI_ERROR("%s: line %lld: a PAF line has at least 9 tab-separated columns. Had %d.", path, line_no, nf);
            exit(EXIT_FAILURE);
        }
        const int32_t start = hap_coord(fs[7], fe[7], path, line_no, 8), finish = hap_coord(fs[8], fe[8], path, line_no, 9);
        if (finish <= start) {
            CLI_ERROR("%s: line %lld: target end %d is not behind target start %d", path, line_no, finish, start);
            exit(EXIT_FAILURE);
        }
        line[fe[5] - line] = 0;
        const int32_t ctg = find_ctg(fs[5], arg);
        if (ctg < 0) { /* a target the assembly BED does not have: `bedtools subtract -a assembly` never sees it */
            ++*n_dropped;
            continue;
        }
        int added;
        const int32_t q = cli_map_put(&queries, fs[0], (size_t)(fe[0] - fs[0]), &added);
        if (*n == *cap) {
            *cap = *cap ? *cap * 2 : 1024;
            *rows = (cornetto_hap_row_t *)cli_xrealloc(*rows, (size_t)*cap * sizeof(**rows));
        }
        cornetto_hap_row_t *r = &(*rows)[(*n)++];
        r->query = q;
        r->ctg = ctg;
        r->start = start;
        r->finish = finish;
        ++n_used;
    }
    free(line);
    fclose(fp);
    cli_map_free(&queries);
    return n_used;
}

/* ---------------------------------------------------------------- the telomere BED */
void cli_telobed_load(const char *path, void (*on_row)(const char *ctg, void *arg), void *arg)
{
    FILE *fp = cli_fopen_chk(path, "r");
    char *line = NULL, *ctg = NULL;
    size_t cap = 0, ctg_cap = 0;
    ssize_t got;
    int64_t line_no = 0;
    while ((got = getline(&line, &cap, fp)) != -1) {
        if ((size_t)got + 1 > ctg_cap) {
            ctg_cap = (size_t)got + 1;
            ctg = (char *)cli_xrealloc(ctg, ctg_cap);
        }
        long beg = -1, end = -1;
        /* (scanf's "\t" skips any white space, as the reference's format does) */
        if (sscanf(line, "%s\t%ld\t%ld", ctg, &beg, &end) != 3 || end < beg) {
            CLI_ERROR("Malformed bed entry at line %lld", (long long)line_no);
            exit(EXIT_FAILURE);
        }
        if (beg < 0 || end < 0) {
            CLI_ERROR("Malformed bed entry at %s:%lld. Coordinates cannot be negative", path, (long long)line_no);
            exit(EXIT_FAILURE);
        }
        if (beg >= end) {
            CLI_ERROR("Malformed bed entry at %s:%lld. start must be smaller than end coordinate", path, (long long)line_no);
            exit(EXIT_FAILURE);
        }
        on_row(ctg, arg);
        ++line_no;
    }
    CLI_VERBOSE("%lld bed entries loaded from %s", (long long)line_no, path);
    free(line);
    free(ctg);
    fclose(fp);
}

/* ---------------------------------------------------------------- natural order */
static int dig(unsigned char c) { return c >= '0' && c <= '9'; }

int cli_strnum_cmp(const char *a_, const char *b_)
{
    const unsigned char *a = (const unsigned char *)a_, *b = (const unsigned char *)b_;
    while (*a && *b) {
        if (!dig(*a) || !dig(*b)) {        /* a character against a character */
            if (*a != *b) return (int)*a - (int)*b;
            ++a;
            ++b;
            continue;
        }
        /* two digit runs: without their leading zeros, the longer run is the larger number; of two equally long ones, the first
         * differing character decides (what stands right after the runs included, when they are equal) */
        while (*a == '0') ++a;
        while (*b == '0') ++b;
        while (dig(*a) && *a == *b) ++a, ++b;
        const int first_diff = (int)*a - (int)*b;
        while (dig(*a) && dig(*b)) ++a, ++b;
        if (dig(*a)) return 1;
        if (dig(*b)) return -1;
        if (first_diff) return first_diff;
    }
    return *a ? 1 : *b ? -1 : 0;
}
