/* fixasm_main.c — `cornetto fixasm`: every contig of an assembly that a PAF of it against a reference names is renamed after the
 * reference sequence most of its alignments hit and turned onto the strand that most of their target bases lie on.  Reference:
 * src/fixasm.c:226-284 (load_paf), :287-338 (write_corrected_paf), :341-405 (fix_the_assembly), :419-480 (options), with the PAF
 * fields of src/pafrec.c:43-98.
 *
 * The PAF side (O(lines)) runs here on the host, with the parser of cli/tables.c.  The FASTA side goes through stream_records() (stream.c): the records are framed on
 * the device, the header lines are built here, and the output text — headers, bases forward or reverse-complemented, newlines — is
 * written on the device window by window (cornetto_emit_*) and copied into pinned slabs that go to stdout with write().
 * CORNETTO_EMIT_SLAB = bytes per window (default 32 MiB; never changes a byte of the output).  CORNETTO_ACCEL=no: the same on the
 * host, record by record (the sequential reader of fastx.c).
 *
 * What the reference does, and this does too: a contig is reversed iff the target bases of its '-' lines outnumber those of its '+'
 * lines (a tie stays '+'); its new name is the target it has the most lines against, the LATER target (in order of first appearance in
 * the PAF) on a tie (:375 compares with >=), with "_PATERNAL" / "_MATERNAL" cut off under --trim-pat-mat, followed by "_k", k counting
 * the records given to that target so far in FASTA order (per target, not per trimmed name).  A FASTA record the PAF does not name is
 * dropped (-m lists it).  A record listed twice is renamed twice; -w takes the last name, and "(null)" (glibc's "%s" of NULL) for a
 * PAF contig the FASTA does not have.  Sequences are printed with "%s" (:384): one that holds a NUL byte is cut there by the reference,
 * not here (outside what this port reproduces). */
#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "cli.h"

/* ---------------------------------------------------------------- the state of a run */
typedef struct {
    int64_t sump, sumn;
    int32_t *tgt, *cnt;   /* lines against each target this contig has (ctg_t.tally of :67-79, kept sparse) */
    int32_t n_t, cap_t;
    int32_t best;         /* the chosen target */
    int rc;
    char *new_name;       /* set by the last FASTA record of this name */
} fx_ctg_t;

typedef struct {
    cli_map_t ctgs, tgts;
    fx_ctg_t *ctg;
    size_t ctg_cap;
    char **clean;          /* target names, trimmed under --trim-pat-mat (cleanup_str, :57-71) */
    int32_t *counter;      /* chr_list_t.counters: records given to each target so far */
    FILE *fp_report, *fp_missing;
    int total, neg, missing;
    /* device path: the pinned slabs of the output windows */
    char *pin[4];
    int64_t pin_cap;
    int64_t slab;
    /* host path: the reverse-complement buffer */
    char *rcbuf;
    size_t rcbuf_cap;
} fx_run_t;

static void fx_load_paf(fx_run_t *R, const char *paf)
{
    FILE *fp = cli_fopen_chk(paf, "r");
    char *line = NULL;
    size_t cap = 0;
    cli_paf_t r;
    while (getline(&line, &cap, fp) != -1) {
        cli_paf_parse(line, &r);
        int added;
        const int32_t ci = cli_map_put(&R->ctgs, r.rid, strlen(r.rid), &added);
        if (added) {
            if ((size_t)ci >= R->ctg_cap) {
                R->ctg_cap = R->ctg_cap ? R->ctg_cap * 2 : 256;
                R->ctg = (fx_ctg_t *)cli_xrealloc(R->ctg, R->ctg_cap * sizeof(fx_ctg_t));
            }
            memset(&R->ctg[ci], 0, sizeof(fx_ctg_t));
        }
        const int32_t ti = cli_map_put(&R->tgts, r.tid, strlen(r.tid), &added);
        fx_ctg_t *c = &R->ctg[ci];
        const int32_t length = (int32_t)((uint32_t)r.te - (uint32_t)r.ts);   /* int32_t difference (:268), wrapping */
        if (r.strand == 0) c->sump += length;
        else c->sumn += length;
        int32_t k = c->n_t - 1;
        if (k < 0 || c->tgt[k] != ti)
            for (k = 0; k < c->n_t && c->tgt[k] != ti; ++k) {}
        if (k == c->n_t) {
            if (c->n_t == c->cap_t) {
                c->cap_t = c->cap_t ? c->cap_t * 2 : 4;
                c->tgt = (int32_t *)cli_xrealloc(c->tgt, (size_t)c->cap_t * sizeof(int32_t));
                c->cnt = (int32_t *)cli_xrealloc(c->cnt, (size_t)c->cap_t * sizeof(int32_t));
            }
            c->tgt[k] = ti;
            c->cnt[k] = 0;
            c->n_t++;
        }
        c->cnt[k]++;
    }
    free(line);
    fclose(fp);
    for (size_t i = 0; i < R->ctgs.n; ++i) {
        fx_ctg_t *c = &R->ctg[i];
        c->rc = c->sump < c->sumn;
        /* the most lines; on a tie the later target (:371-378 walks every target index with >=) */
        c->best = -1;
        int32_t most = -1;
        for (int32_t k = 0; k < c->n_t; ++k)
            if (c->cnt[k] > most || (c->cnt[k] == most && c->tgt[k] > c->best)) {
                most = c->cnt[k];
                c->best = c->tgt[k];
            }
    }
}

static void fx_trim_names(fx_run_t *R, int trim)
{
    R->clean = (char **)cli_xmalloc((R->tgts.n + 1) * sizeof(char *));
    R->counter = (int32_t *)calloc(R->tgts.n + 1, sizeof(int32_t));
    if (!R->counter) { CLI_ERROR("Failed to allocate memory: %s", strerror(errno)); exit(EXIT_FAILURE); }
    for (size_t t = 0; t < R->tgts.n; ++t) {
        char *s = cli_xstrdup(R->tgts.keys[t]);
        if (trim) {
            char *p = strstr(s, "_PATERNAL");
            if (p) *p = 0;
            p = strstr(s, "_MATERNAL");
            if (p) *p = 0;
        }
        R->clean[t] = s;
    }
}

/* one FASTA record: -1 if the PAF does not name it (then listed in -m), else its contig; *head gets ">new_name\n" */
static int32_t fx_name(fx_run_t *R, const char *name, size_t name_len, char **head, size_t *head_len)
{
    const int32_t ci = cli_map_get(&R->ctgs, name, name_len);
    if (ci < 0) {
        if (R->fp_missing) {
            fwrite(name, 1, name_len, R->fp_missing);
            fputc('\n', R->fp_missing);
        }
        R->missing++;
        return -1;
    }
    fx_ctg_t *c = &R->ctg[ci];
    const char *chr = R->clean[c->best];
    const int32_t k = R->counter[c->best]++;
    const size_t cl = strlen(chr);
    free(c->new_name);
    c->new_name = (char *)cli_xmalloc(cl + 16);
    const int nn = snprintf(c->new_name, cl + 16, "%s_%d", chr, k);
    if (R->fp_report) {
        fwrite(name, 1, name_len, R->fp_report);
        fprintf(R->fp_report, "\t%s\t%c\t%s\n", chr, c->rc ? '-' : '+', c->new_name);
    }
    *head = c->new_name;
    *head_len = (size_t)nn;
    R->total++;
    if (c->rc) R->neg++;
    return ci;
}

static void fx_write_all(const char *p, int64_t n)
{
    while (n > 0) {
        const ssize_t w = write(STDOUT_FILENO, p, (size_t)(n > (1LL << 30) ? (1LL << 30) : n));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            CLI_ERROR("writing the output failed: %s", strerror(errno));
            exit(EXIT_FAILURE);
        }
        p += w;
        n -= w;
    }
}

/* ---------------------------------------------------------------- the device path: one batch of framed records */
#define FX_SLOTS 4

static void fixasm_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n_rec, const cornetto_asm_t *a, void *arg)
{
    fx_run_t *R = (fx_run_t *)arg;
    cornetto_emit_rec_t *er = (cornetto_emit_rec_t *)cli_xmalloc(((size_t)n_rec + 1) * sizeof(*er));
    size_t heads_cap = 4096, n_heads = 0, n_er = 0;
    char *heads = (char *)cli_xmalloc(heads_cap);
    for (int64_t i = 0; i < n_rec; ++i) {
        char *nm;
        size_t nl;
        const int32_t ci = fx_name(R, r[i].name, (size_t)r[i].name_len, &nm, &nl);
        if (ci < 0) continue;
        if (n_heads + nl + 2 > heads_cap) {
            while (n_heads + nl + 2 > heads_cap) heads_cap *= 2;
            heads = (char *)cli_xrealloc(heads, heads_cap);
        }
        er[n_er].ctg = (int32_t)i;
        er[n_er].rc = R->ctg[ci].rc;
        er[n_er].head = (int64_t)n_heads;
        er[n_er].head_len = (int64_t)nl + 2;
        heads[n_heads++] = '>';
        memcpy(heads + n_heads, nm, nl);
        n_heads += nl;
        heads[n_heads++] = '\n';
        n_er++;
    }
    if (n_er) {
        cornetto_emit_t *e = NULL;
        int64_t total = 0;
        cli_accel_check(h, cornetto_emit_open(h, a, er, (int64_t)n_er, heads, (int64_t)n_heads, &e, &total), "planning the output text");
        const int64_t S = R->slab < total ? R->slab : total;
        if (R->pin_cap < S) {
            for (int s = 0; s < FX_SLOTS; ++s) {
                if (R->pin[s]) cornetto_pinned_free(R->pin[s]);
                R->pin[s] = (char *)cornetto_pinned_alloc((size_t)S);
                if (!R->pin[s]) {
                    CLI_ERROR("could not allocate a %lld-byte pinned slab", (long long)S);
                    exit(EXIT_FAILURE);
                }
            }
            R->pin_cap = S;
        }
        fflush(stdout);
        const int64_t nw = (total + S - 1) / S;
        /* window w on slot w % 4: its kernel and copy run while the window before it is written out */
        for (int64_t w = 0; w < nw + FX_SLOTS; ++w) {
            if (w >= FX_SLOTS && w - FX_SLOTS < nw) {
                const int64_t v = w - FX_SLOTS, at = v * S, len = total - at < S ? total - at : S;
                cli_accel_check(h, cornetto_emit_wait(h, e, (int)(v % FX_SLOTS)), "writing the output text");
                fx_write_all(R->pin[v % FX_SLOTS], len);
            }
            if (w < nw) {
                const int64_t at = w * S, len = total - at < S ? total - at : S;
                cli_accel_check(h, cornetto_emit_get(h, e, R->pin[w % FX_SLOTS], at, len, (int)(w % FX_SLOTS)), "writing the output text");
            }
        }
        cornetto_emit_free(h, e);
    }
    free(heads);
    free(er);
}

/* ---------------------------------------------------------------- the host path (CORNETTO_ACCEL=no) */
static void fx_host_fasta(fx_run_t *R, const char *path)
{
    cli_fastx_t *fx = cli_fastx_open(path, 1);
    cli_rec_t *r;
    while ((r = cli_fastx_next_checked(fx)) != NULL) {
        const int64_t l = (int64_t)r->seq.l;
        char *nm;
        size_t nl;
        const int32_t ci = fx_name(R, r->name.s, r->name.l, &nm, &nl);
        if (ci < 0) continue;
        const char *s = r->seq.s;
        if (R->ctg[ci].rc) {   /* reverse_complement(), :208-224 */
            if ((size_t)l + 1 > R->rcbuf_cap) {
                R->rcbuf_cap = (size_t)l + 1;
                R->rcbuf = (char *)cli_xrealloc(R->rcbuf, R->rcbuf_cap);
            }
            for (int64_t i = 0; i < l; ++i) {
                const char c = s[l - 1 - i];
                R->rcbuf[i] = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'C' ? 'G' : c;
            }
            s = R->rcbuf;
        }
        fputc('>', stdout);
        fwrite(nm, 1, nl, stdout);
        fputc('\n', stdout);
        fwrite(s, 1, (size_t)l, stdout);
        fputc('\n', stdout);
    }
    cli_fastx_close(fx);
}

/* ---------------------------------------------------------------- -w (write_corrected_paf, :287-338) */
static void fx_write_paf(const fx_run_t *R, const char *out_paf, const char *paf)
{
    FILE *fp = cli_fopen_chk(paf, "r");
    FILE *fw = cli_fopen_chk(out_paf, "w");
    char *line = NULL;
    size_t cap = 0;
    cli_paf_t r;
    while (getline(&line, &cap, fp) != -1) {
        cli_paf_parse(line, &r);
        const int32_t ci = cli_map_get(&R->ctgs, r.rid, strlen(r.rid));
        if (ci < 0) {   /* (the file changed since it was loaded) */
            fprintf(stderr, "Error: contig %s not found in hash table\n", r.rid);
            exit(EXIT_FAILURE);
        }
        const fx_ctg_t *c = &R->ctg[ci];
        int dir = r.strand;
        int32_t qs = r.qs, qe = r.qe;
        if (c->rc) {
            dir = !dir;
            qs = (int32_t)((uint32_t)r.qlen - (uint32_t)r.qe);
            qe = (int32_t)((uint32_t)r.qlen - (uint32_t)r.qs);
        }
        fprintf(fw, "%s\t%d\t%d\t%d\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:%c\n", c->new_name ? c->new_name : "(null)", r.qlen, qs, qe,
                dir == 0 ? '+' : '-', r.tid, r.tlen, r.ts, r.te, r.match, r.block, (int)r.mapq, r.tp);
    }
    free(line);
    fclose(fp);
    fclose(fw);
}

static const struct option fx_long[] = {
    {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {"missing", required_argument, 0, 'm'},
    {"report", required_argument, 0, 'r'},  {"trim-pat-mat", no_argument, 0, 0}, {0, 0, 0, 0}};

static void fx_help(FILE *fp)
{
    fprintf(fp, "Usage: cornetto fixasm <assembly.fa> <asm_to_ref.paf>\n");
    fprintf(fp, "   -m FILE                    write missing contig names to FILE\n");
    fprintf(fp, "   -r FILE                    write report to FILE\n");
    fprintf(fp, "   -w FILE                    write fixed PAF to FILE\n");
    fprintf(fp, "   -v INT                     verbosity level [%d]\n", cli_log_level);
    fprintf(fp, "   -h                         help\n");
}

int fixasm_main(int argc, char *argv[])
{
    const char *missing = NULL, *report = NULL, *out_paf = NULL;
    int trim = 0, c, li = 0;
    FILE *fp_help = stderr;
    optind = 1;
    while ((c = getopt_long(argc, argv, "v:r:m:w:h", fx_long, &li)) >= 0) {
        if (c == 'm') missing = optarg;
        else if (c == 'r') report = optarg;
        else if (c == 'w') out_paf = optarg;
        else if (c == 'v') cli_log_level = atoi(optarg);
        else if (c == 'h') fp_help = stdout;
        else if (c == 0 && li == 4) trim = 1;
    }
    if (argc - optind != 2) {   /* -h alone ends here too, with status 1 (:455-458) */
        fx_help(fp_help);
        exit(EXIT_FAILURE);
    }
    const char *fasta = argv[optind], *paf = argv[optind + 1];

    fx_run_t R;
    memset(&R, 0, sizeof(R));
    fx_load_paf(&R, paf);
    fx_trim_names(&R, trim);
    gzclose((gzFile)cli_gz_open(fasta, 1));   /* the FASTA is opened before the report and missing files (:343-356) */
    if (report) R.fp_report = cli_fopen_chk(report, "w");
    if (missing) R.fp_missing = cli_fopen_chk(missing, "w");

    if (cli_host_mode()) {
        fx_host_fasta(&R, fasta);
    } else {
        const char *e = getenv("CORNETTO_EMIT_SLAB");
        R.slab = e ? atoll(e) : 0;
        if (R.slab < 1) R.slab = 32LL << 20;
        int devs[CLI_MAX_DEV];
        if (cli_device_list(devs) >= 1) {   /* one device: the first listed */
            char one[32];
            snprintf(one, sizeof(one), "%d", devs[0]);
            setenv("CORNETTO_DEVICE", one, 1);
        }
        stream_records(fasta, 1, fixasm_scan, &R, 0);
    }
    fflush(stdout);
    fprintf(stderr, "total: %d\nnegative: %d\nmissing: %d\n", R.total, R.neg, R.missing);
    if (R.fp_report) fclose(R.fp_report);
    if (R.fp_missing) fclose(R.fp_missing);
    if (out_paf) fx_write_paf(&R, out_paf, paf);
    return 0;
}
