/* eval_main.c — the evaluation sub-commands of the assembly toolkit: nx (src/nx.c), report (src/report.c), telocontigs
 * (src/telocontigs.c) and asmstats (src/asmstats.c).  Same options, stdout bytes and exit codes as the reference.
 *
 * Every FASTA/FASTQ(+gz) input is read through stream_names() (stream.c): the records are framed on the device with no bases
 * materialised, one device handle serving all files of the process (report reads one assembly per iteration); CORNETTO_ACCEL=no reads
 * them with the sequential reader.  The tables (telomere BED, fixasm report, PAF) are parsed on the host (tables.c).
 *
 * Where this differs from the reference on purpose:
 *  - telocontigs prints the telomere counts the program means.  The reference keeps pointers into its contig array in its hash table and
 *    moves that array with realloc() when the FASTA has more than 100 records (src/telocontigs.c:199): from then on the counts of the
 *    records before the last growth go to freed memory (lost, or a corrupted heap and SIGABRT).  Its output is the same as this one
 *    wherever the array did not move under a BED row: 100 records or fewer, or rows only on records at index >= 100 * 2^k of its last growth.
 *  - the reference's asserts are not imitated: a NUL byte inside a record (src/nx.c:129 and the like), a target name that
 *    --trim-pat-mat cuts down to nothing (src/asmstats.c:169).  These inputs are read like any other. */
#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>

#include "cli.h"

/* ---------------------------------------------------------------- records of a FASTA/FASTQ file */
typedef struct {
    int64_t *len;
    char **name;        /* only if want_names */
    int64_t n, cap;
    int want_names;
} recs_t;

static void take_names(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    (void)h;
    (void)a;
    recs_t *R = (recs_t *)arg;
    for (int64_t i = 0; i < n; ++i) {
        if (r[i].len > 0x7fffffffLL) {
            CLI_ERROR("a record has %lld bases; the reference's reader is limited to 2^31-1 (src/kseq.h:185)", (long long)r[i].len);
            exit(EXIT_FAILURE);
        }
        if (R->n == R->cap) {
            R->cap = R->cap ? R->cap * 2 : 1024;
            R->len = (int64_t *)cli_xrealloc(R->len, (size_t)R->cap * sizeof(int64_t));
            if (R->want_names) R->name = (char **)cli_xrealloc(R->name, (size_t)R->cap * sizeof(char *));
        }
        R->len[R->n] = r[i].len;
        if (R->want_names) {
            char *s = (char *)cli_xmalloc((size_t)r[i].name_len + 1);
            memcpy(s, r[i].name, (size_t)r[i].name_len);
            s[r[i].name_len] = 0;
            R->name[R->n] = s;
        }
        R->n++;
    }
}

/* every record of `path` (the reference's F_CHK exit if it cannot be opened) */
static void read_records(const char *path, int want_names, recs_t *R)
{
    memset(R, 0, sizeof(*R));
    R->want_names = want_names;
    stream_names(path, 1, take_names, R);
}

static void recs_free(recs_t *R)
{
    if (R->name)
        for (int64_t i = 0; i < R->n; ++i) free(R->name[i]);
    free(R->name);
    free(R->len);
}

static int cmp_i64(const void *a, const void *b)
{
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return x < y ? -1 : x > y;
}

static const struct option help_only[] = {{"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

/* ---------------------------------------------------------------- nx */
/* mm_parse_num (src/misc.c:72-84): a number with an optional G / M / K suffix, rounded */
static int64_t parse_num(const char *s)
{
    char *p;
    double x = strtod(s, &p);
    if (*p == 'G' || *p == 'g') x *= 1e9;
    else if (*p == 'M' || *p == 'm') x *= 1e6;
    else if (*p == 'K' || *p == 'k') x *= 1e3;
    return (int64_t)(x + .499);
}

int nx_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"genome-size", required_argument, 0, 'g'}, {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    FILE *fp_help = stderr;
    int64_t genome = -1;
    int c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "g:h", lo, &li)) >= 0) {
        if (c == 'h') {
            fp_help = stdout;
        } else if (c == 'g') {
            genome = parse_num(optarg);
            if (genome <= 0) {
                CLI_ERROR("%s", "Genome size should be larger than 0.");
                exit(EXIT_FAILURE);
            }
        }
    }
    if (argc - optind != 1 || fp_help == stdout) {
        fprintf(fp_help, "Usage: cornetto nx <assembly.fasta> \n");
        fprintf(fp_help, "   -g STR                     genome size (e.g. 3.1G). if unspecified, will use total contig length\n");
        fprintf(fp_help, "   -h                         help\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    recs_t R;
    read_records(argv[optind], 0, &R);
    uint64_t sum = 0;
    for (int64_t i = 0; i < R.n; ++i) sum += (uint64_t)R.len[i];
    if (R.n) qsort(R.len, (size_t)R.n, sizeof(int64_t), cmp_i64);
    fputs("#x\tcontig_len\n", stdout);
    /* per record, longest first: the percent before it and after it (an all-empty file divides 0 by 0: "-nan", as the reference prints) */
    uint64_t cum = 0;
    double pct = 0;
    for (int64_t i = R.n - 1; i >= 0; --i) {
        const uint64_t l = (uint64_t)R.len[i];
        printf("%f\t%lu\n", pct, (unsigned long)l);
        cum += l;
        pct = genome > 0 ? (double)cum / (double)genome * 100 : (double)cum / (double)sum * 100;
        printf("%f\t%lu\n", pct, (unsigned long)l);
    }
    recs_free(&R);
    return 0;
}

/* ---------------------------------------------------------------- report */
int report_main(int argc, char *argv[])
{
    FILE *fp_help = stderr;
    int c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "h", help_only, &li)) >= 0)
        if (c == 'h') fp_help = stdout;
    if (argc - optind < 1 || fp_help == stdout) {
        fprintf(fp_help, "Usage: cornetto report <assembly.fasta> ... \n");
        fprintf(fp_help, "   -h                         help\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    fputs("#asm\tNcontigs\tLargestcontig(Mbase)\tN50(Mbase)\tN90(Mbase)\n", stdout);
    for (int k = optind; k < argc; ++k) {
        /* the name goes out before the file is opened: a missing file leaves "name\t" on stdout (exit() flushes it) */
        printf("%s\t", argv[k]);
        recs_t R;
        read_records(argv[k], 0, &R);
        if (R.n == 0) {
            /* the reference prints length[-1] of its empty 100-entry array as the longest record: glibc's chunk header of that 800-byte
             * block, 0x331 = 817 (src/report.c:149) */
            printf("0\t%.3f\t%.3f\t%.3f\n", 817 / 1e6, 0 / 1e6, 0 / 1e6);
            recs_free(&R);
            continue;
        }
        uint64_t sum = 0;
        for (int64_t i = 0; i < R.n; ++i) sum += (uint64_t)R.len[i];
        qsort(R.len, (size_t)R.n, sizeof(int64_t), cmp_i64);
        /* N50 / N90: the first record, longest first, at which the running sum reaches half / nine tenths of the total (in double) */
        uint64_t cum = 0, n50 = 0, n90 = 0;
        for (int64_t i = R.n - 1; i >= 0; --i) {
            const uint64_t l = (uint64_t)R.len[i];
            cum += l;
            if ((double)cum >= (double)sum * 0.5 && n50 == 0) n50 = l;
            if ((double)cum >= (double)sum * 0.9 && n90 == 0) n90 = l;
        }
        printf("%ld\t%.3f\t%.3f\t%.3f\n", (long)R.n, (double)R.len[R.n - 1] / 1e6, (double)n50 / 1e6, (double)n90 / 1e6);
        recs_free(&R);
    }
    return 0;
}

/* ---------------------------------------------------------------- telocontigs */
typedef struct {
    cli_map_t names;
    uint32_t *ntelo;
} telo_ctx_t;

static void telocontigs_row(const char *ctg, void *arg)
{
    telo_ctx_t *T = (telo_ctx_t *)arg;
    const int32_t i = cli_map_get(&T->names, ctg, strlen(ctg));
    if (i < 0) {
        CLI_ERROR("Contig '%s' in bed file not found in fasta", ctg);
        exit(EXIT_FAILURE);
    }
    T->ntelo[i]++;
}

int telocontigs_main(int argc, char *argv[])
{
    FILE *fp_help = stderr;
    int c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "h", help_only, &li)) >= 0)
        if (c == 'h') fp_help = stdout;
    if (argc - optind != 2 || fp_help == stdout) {
        fprintf(fp_help, "Usage: cornetto telocontigs <assembly.fasta> <telomere.bed>\n");
        fprintf(fp_help, "   -h                         help\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    recs_t R;
    read_records(argv[optind], 1, &R);
    if (R.n > 0x7ffffffeLL) {
        CLI_ERROR("%s", "more than 2^31-2 records");
        exit(EXIT_FAILURE);
    }
    telo_ctx_t T;
    memset(&T, 0, sizeof(T));
    T.ntelo = (uint32_t *)calloc((size_t)R.n + 1, sizeof(uint32_t));
    if (!T.ntelo) { CLI_ERROR("Failed to allocate memory: %s", strerror(errno)); exit(EXIT_FAILURE); }
    for (int64_t i = 0; i < R.n; ++i) {
        int added;
        (void)cli_map_put(&T.names, R.name[i], strlen(R.name[i]), &added);
        if (!added) {
            CLI_ERROR("Duplicate contig '%s' found in fasta", R.name[i]);
            exit(EXIT_FAILURE);
        }
    }
    cli_telobed_load(argv[optind + 1], telocontigs_row, &T);
    /* longest first, equal lengths in input order (glibc's qsort is a stable merge sort here) */
    int32_t *order = (int32_t *)cli_xmalloc(((size_t)R.n + 1) * sizeof(int32_t));
    cli_order_by_length_desc(R.len, NULL, (int32_t)R.n, order);
    fputs("Contig\tLength\tNTelomeres\n", stdout);
    for (int64_t k = 0; k < R.n; ++k) {
        const int32_t i = order[k];
        printf("%s\t%lu\t%u\n", R.name[i], (unsigned long)R.len[i], T.ntelo[i]);
    }
    free(order);
    free(T.ntelo);
    cli_map_free(&T.names);
    recs_free(&R);
    return 0;
}

/* ---------------------------------------------------------------- asmstats */
typedef struct {
    uint32_t ntelo;
    uint32_t len;      /* qlen of its first PAF record (0: none) */
    int32_t chr;       /* the chromosome the fixasm report gives it (an id of `names`), -1: none */
    int64_t n_recs;    /* PAF records */
} as_ctg_t;

typedef struct {
    int32_t tid, ctg;  /* target (an id of `names`), contig */
    uint64_t ta;       /* aligned target bases: te - ts per record, as uint32, summed (after the merge of one contig's records) */
} as_rec_t;

typedef struct {
    cli_map_t ctgs;    /* contigs: the keys of the reference's h_ctg (BED names, then the report's contigs) in order of insertion */
    as_ctg_t *ctg;
    size_t ctg_cap;
    cli_map_t chrs;    /* the report's chromosomes (h_chr) */
    uint32_t *chr_len; /* tlen of the first PAF record on it (0: none) */
    size_t chr_cap;
    cli_map_t names;   /* every chromosome / target name a comparison meets: equal strings have equal ids */
    as_rec_t *rec;
    int64_t n_rec, cap_rec;
} as_run_t;

static int32_t as_ctg_put(as_run_t *A, const char *name)
{
    int added;
    const int32_t i = cli_map_put(&A->ctgs, name, strlen(name), &added);
    if (added) {
        if ((size_t)i >= A->ctg_cap) {
            A->ctg_cap = A->ctg_cap ? A->ctg_cap * 2 : 256;
            A->ctg = (as_ctg_t *)cli_xrealloc(A->ctg, A->ctg_cap * sizeof(as_ctg_t));
        }
        A->ctg[i].ntelo = 0;
        A->ctg[i].len = 0;
        A->ctg[i].chr = -1;
        A->ctg[i].n_recs = 0;
    }
    return i;
}

static int32_t as_name(as_run_t *A, const char *s)
{
    int added;
    return cli_map_put(&A->names, s, strlen(s), &added);
}

static void as_bed_row(const char *ctg, void *arg)
{
    as_run_t *A = (as_run_t *)arg;
    const int32_t i = as_ctg_put(A, ctg);   /* (may move A->ctg) */
    A->ctg[i].ntelo++;
}

/* load_fixasm_report (src/asmstats.c:292-370): "<ctg> <chr> ..." per line; a contig listed again takes the later chromosome */
static void as_load_report(as_run_t *A, const char *path)
{
    FILE *fp = cli_fopen_chk(path, "r");
    char *line = NULL, *ctg = NULL, *chr = NULL;
    size_t cap = 0, tok_cap = 0;
    ssize_t got;
    int64_t line_no = 0;
    while ((got = getline(&line, &cap, fp)) != -1) {
        if ((size_t)got + 1 > tok_cap) {
            tok_cap = (size_t)got + 1;
            ctg = (char *)cli_xrealloc(ctg, tok_cap);
            chr = (char *)cli_xrealloc(chr, tok_cap);
        }
        if (sscanf(line, "%s\t%s", ctg, chr) != 2) {
            CLI_ERROR("Malformed report entry at line %lld. Expected format: <ctg>\t<chr>", (long long)line_no);
            exit(EXIT_FAILURE);
        }
        const int32_t ci = as_ctg_put(A, ctg);
        A->ctg[ci].chr = as_name(A, chr);
        int added;
        const int32_t k = cli_map_put(&A->chrs, chr, strlen(chr), &added);
        if (added) {
            if ((size_t)k >= A->chr_cap) {
                A->chr_cap = A->chr_cap ? A->chr_cap * 2 : 64;
                A->chr_len = (uint32_t *)cli_xrealloc(A->chr_len, A->chr_cap * sizeof(uint32_t));
            }
            A->chr_len[k] = 0;
        }
        ++line_no;
    }
    free(line);
    free(ctg);
    free(chr);
    fclose(fp);
}

/* load_paf (src/asmstats.c:172-228) */
static void as_load_paf(as_run_t *A, const char *path, int trim)
{
    FILE *fp = cli_fopen_chk(path, "r");
    char *line = NULL;
    size_t cap = 0;
    cli_paf_t r;
    while (getline(&line, &cap, fp) != -1) {
        cli_paf_parse(line, &r);
        if (trim) {
            char *p = strstr(r.tid, "_PATERNAL");
            if (p) *p = 0;
            p = strstr(r.tid, "_MATERNAL");
            if (p) *p = 0;
        }
        const int32_t ci = cli_map_get(&A->ctgs, r.rid, strlen(r.rid));
        if (ci < 0) {
            CLI_WARNING("Contig '%s' in PAF file was not there in the tsv report or the telomere bed", r.rid);
            continue;
        }
        as_ctg_t *c = &A->ctg[ci];
        if (c->len == 0) {
            c->len = (uint32_t)r.qlen;
        } else if (c->len != (uint32_t)r.qlen) {
            CLI_ERROR("Contig '%s' has inconsistent lengths in PAF file", r.rid);
            exit(EXIT_FAILURE);
        }
        if (A->n_rec == A->cap_rec) {
            A->cap_rec = A->cap_rec ? A->cap_rec * 2 : 1024;
            A->rec = (as_rec_t *)cli_xrealloc(A->rec, (size_t)A->cap_rec * sizeof(as_rec_t));
        }
        as_rec_t *e = &A->rec[A->n_rec++];
        e->tid = as_name(A, r.tid);
        e->ctg = ci;
        e->ta = (uint32_t)r.te - (uint32_t)r.ts;     /* int32_t difference stored as uint32_t (:471), wrapping */
        c->n_recs++;
        const int32_t k = cli_map_get(&A->chrs, r.tid, strlen(r.tid));
        if (k >= 0) {
            if (A->chr_len[k] == 0) {
                A->chr_len[k] = (uint32_t)r.tlen;
            } else if (A->chr_len[k] != (uint32_t)r.tlen) {
                CLI_ERROR("Chromosome '%s' has inconsistent lengths in PAF file", r.tid);
                exit(EXIT_FAILURE);
            }
        } else {
            CLI_WARNING("Chromosome '%s' in PAF file was not there in the tsv report or the telomere bed", r.tid);
        }
    }
    free(line);
    fclose(fp);
}

static int cmp_rec(const void *a, const void *b)
{
    const as_rec_t *x = (const as_rec_t *)a, *y = (const as_rec_t *)b;
    if (x->tid != y->tid) return x->tid < y->tid ? -1 : 1;
    return x->ctg < y->ctg ? -1 : x->ctg > y->ctg;
}

static int cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

static char **g_sort_names;
static int cmp_chr_idx(const void *a, const void *b)   /* strnum order of g_sort_names[], ties by index (a stable sort) */
{
    const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
    const int d = cli_strnum_cmp(g_sort_names[x], g_sort_names[y]);
    return d ? d : (x < y ? -1 : x > y);
}

/* khash bucket order of the distinct keys of `m` inserted in index order -> ids (n = m->n) */
static int32_t *bucket_order(const cli_map_t *m)
{
    int32_t *slot = (int32_t *)cli_xmalloc((m->n + 1) * sizeof(int32_t)), *order = (int32_t *)cli_xmalloc((m->n + 1) * sizeof(int32_t));
    if (cornetto_khash_str_order((const char *const *)m->keys, (int32_t)m->n, slot, order) != (int32_t)m->n) {
        CLI_ERROR("%s", "khash order: bad argument");
        exit(EXIT_FAILURE);
    }
    free(slot);
    return order;
}

static void pct5(const uint64_t *s, uint32_t len, char sep)
{
    for (int k = 0; k < 5; ++k) printf("%.3f%c", (double)s[k] / len * 100, k < 4 ? sep : '\n');
}

int asmstats_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"report", required_argument, 0, 'r'}, {"sort-order", required_argument, 0, 's'}, {"trim-pat-mat", no_argument, 0, 0},
                                       {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    FILE *fp_help = stderr;
    const char *report = NULL, *sort_order = NULL;
    int trim = 0, c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "r:s:h", lo, &li)) >= 0) {
        if (c == 'h') fp_help = stdout;
        else if (c == 'r') report = optarg;
        else if (c == 's') sort_order = optarg;
        else if (c == 0 && li == 2) trim = 1;
    }
    if (argc - optind != 2 || fp_help == stdout || !report) {
        fprintf(fp_help, "Usage: cornetto asmstats <asm2ref.paf> <telomere.bed> -r <fixasm.report.tsv>\n");
        fprintf(fp_help, "   -r FILE                    report file generated from fixasm\n");
        fprintf(fp_help, "   -s STR                     use the sort order specified by STR when printing the chromosome report (human1 for haploid human, human2 for diploid human or ref.fasta)\n");
        fprintf(fp_help, "   -v INT                     verbosity level [%d]\n", cli_log_level);
        fprintf(fp_help, "   -h                         help\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    const char *paf = argv[optind], *bed = argv[optind + 1];
    as_run_t A;
    memset(&A, 0, sizeof(A));
    cli_telobed_load(bed, as_bed_row, &A);
    as_load_report(&A, report);
    as_load_paf(&A, paf, trim);

    /* the chromosomes to print */
    char **list = NULL;
    int64_t n_list = 0;
    recs_t ref;
    memset(&ref, 0, sizeof(ref));
    char human[46][16];
    char *human_p[46];
    if (!sort_order) {
        /* the report's chromosomes in bucket order, then sorted by name (stable: names that compare equal keep their bucket order) */
        int32_t *ord = bucket_order(&A.chrs);
        char **in_buckets = (char **)cli_xmalloc((A.chrs.n + 1) * sizeof(char *));
        for (size_t k = 0; k < A.chrs.n; ++k) {
            in_buckets[k] = A.chrs.keys[ord[k]];
            ord[k] = (int32_t)k;
        }
        g_sort_names = in_buckets;
        qsort(ord, A.chrs.n, sizeof(int32_t), cmp_chr_idx);
        list = (char **)cli_xmalloc((A.chrs.n + 1) * sizeof(char *));
        for (size_t k = 0; k < A.chrs.n; ++k) list[k] = in_buckets[ord[k]];
        n_list = (int64_t)A.chrs.n;
        free(in_buckets);
        free(ord);
    } else if (!strcmp(sort_order, "human1") || !strcmp(sort_order, "human2")) {
        /* human1: chr1..chr22, chrX, chrY; human2: chrN_MATERNAL, chrN_PATERNAL for N = 1..22, then chrX_MATERNAL, chrY_PATERNAL (:45-57) */
        const int two = sort_order[5] == '2';
        for (int k = 1; k <= 22; ++k) {
            if (two) {
                snprintf(human[n_list++], 16, "chr%d_MATERNAL", k);
                snprintf(human[n_list++], 16, "chr%d_PATERNAL", k);
            } else {
                snprintf(human[n_list++], 16, "chr%d", k);
            }
        }
        snprintf(human[n_list++], 16, two ? "chrX_MATERNAL" : "chrX");
        snprintf(human[n_list++], 16, two ? "chrY_PATERNAL" : "chrY");
        for (int64_t k = 0; k < n_list; ++k) human_p[k] = human[k];
        list = human_p;
    } else {
        CLI_VERBOSE("Unknown order: %s. Options are: [human1, human2]. Assuming %s is a reference file", sort_order, sort_order);
        read_records(sort_order, 1, &ref);
        list = ref.name;
        n_list = ref.n;
    }

    /* contigs by chromosome, in the bucket order of h_ctg */
    const size_t n_ctg = A.ctgs.n, n_names = A.names.n;
    int32_t *ctg_order = bucket_order(&A.ctgs);
    int64_t *by_first = (int64_t *)calloc(n_names + 2, sizeof(int64_t));
    int32_t *by_chr = (int32_t *)cli_xmalloc((n_ctg + 1) * sizeof(int32_t));
    if (!by_first) { CLI_ERROR("Failed to allocate memory: %s", strerror(errno)); exit(EXIT_FAILURE); }
    for (size_t i = 0; i < n_ctg; ++i)
        if (A.ctg[i].chr >= 0) by_first[A.ctg[i].chr + 1]++;
    for (size_t t = 0; t < n_names; ++t) by_first[t + 1] += by_first[t];
    {
        int64_t *fill = (int64_t *)cli_xmalloc((n_names + 1) * sizeof(int64_t));
        memcpy(fill, by_first, (n_names + 1) * sizeof(int64_t));
        for (size_t k = 0; k < n_ctg; ++k) {
            const int32_t i = ctg_order[k];
            if (A.ctg[i].chr >= 0) by_chr[fill[A.ctg[i].chr]++] = i;
        }
        free(fill);
    }
    /* aligned bases per (target, contig): the records sorted by target, then contig, and merged */
    if (A.n_rec) qsort(A.rec, (size_t)A.n_rec, sizeof(as_rec_t), cmp_rec);
    int64_t n_run = 0;
    for (int64_t j = 0; j < A.n_rec; ++j) {
        if (n_run && A.rec[n_run - 1].tid == A.rec[j].tid && A.rec[n_run - 1].ctg == A.rec[j].ctg) A.rec[n_run - 1].ta += A.rec[j].ta;
        else A.rec[n_run++] = A.rec[j];
    }
    int64_t *run_first = (int64_t *)calloc(n_names + 2, sizeof(int64_t));
    uint64_t *ta_of = (uint64_t *)calloc(n_ctg + 1, sizeof(uint64_t));
    uint32_t *aln = (uint32_t *)cli_xmalloc((n_ctg + 1) * sizeof(uint32_t));
    if (!run_first || !ta_of) { CLI_ERROR("Failed to allocate memory: %s", strerror(errno)); exit(EXIT_FAILURE); }
    for (int64_t j = 0; j < n_run; ++j) run_first[A.rec[j].tid + 1]++;
    for (size_t t = 0; t < n_names; ++t) run_first[t + 1] += run_first[t];

    printf("%s\n\n", paf);

    /* table 1 (telo_table, :412-481): the contigs of each chromosome that have telomeres */
    fputs("chr\tT2T?\tNTelo\tTelocontiglen\n", stdout);
    for (int64_t i = 0; i < n_list; ++i) {
        const int32_t t = cli_map_get(&A.names, list[i], strlen(list[i]));
        int32_t total = 0, n = 0;
        printf("%s\t", list[i]);
        if (t >= 0) {
            for (int64_t k = by_first[t]; k < by_first[t + 1]; ++k)
                if (A.ctg[by_chr[k]].ntelo > 0) {
                    printf("%c,", A.ctg[by_chr[k]].ntelo == 2 ? 'y' : 'n');
                    total += (int32_t)A.ctg[by_chr[k]].ntelo;
                    ++n;
                }
        }
        if (n > 0) {
            printf("\t%d\t", total);
            for (int64_t k = by_first[t]; k < by_first[t + 1]; ++k)
                if (A.ctg[by_chr[k]].ntelo > 0) printf("%d,", (int32_t)A.ctg[by_chr[k]].len);
        } else {
            fputs("\t\t", stdout);
        }
        fputs("\n", stdout);
    }

    /* tables 2-4 (contig_majority_common, :590-620): 0 = contigs the report puts on the chromosome, 1 = LX of those, 2 = contigs it puts
     * elsewhere.  A chromosome the report does not have is printed alone; one the PAF never reached ends the program (exit 1) */
    static const char *const title[3] = {"Contigs whose majority is mapped to the corresponding chromosome\n",
                                         "LX of Contigs whose majority is mapped to the corresponding chromosome\n",
                                         "Contigs whose majority is mapped to another chromosome\n"};
    for (int table = 0; table < 3; ++table) {
        printf("\n\n%s", title[table]);
        if (table == 1) {
            fputs("\tL50\tL90\tL95\tL99\tCumCovN5\n", stdout);
        } else {
            fputs("\tNcontigsofsize>=KMbasealignedtochr\t\t\t\t\t%ofchrsequencecoveredbycontigsofsize>=KMbase\n", stdout);
            fputs("chr\t0Mbase\t0.1Mbase\t1Mbase\t5Mbase\t10Mbase\t0Mbase\t0.1Mbase\t1Mbase\t5Mbase\t10Mbase\n", stdout);
        }
        for (int64_t i = 0; i < n_list; ++i) {
            const int32_t k = cli_map_get(&A.chrs, list[i], strlen(list[i]));
            if (k < 0) {
                CLI_WARNING("Failed to get chromosome %s from hash table. Ignoring.", list[i]);
                printf("%s\n", list[i]);
                continue;
            }
            const uint32_t len = A.chr_len[k];
            if (len == 0) {
                CLI_ERROR("Failed to get chromosome %s length from hash table. Check your input files.", list[i]);
                exit(EXIT_FAILURE);
            }
            const int32_t t = cli_map_get(&A.names, list[i], strlen(list[i]));   /* (a report chromosome always has a name id) */
            if (table != 1) {
                /* contigs aligned to this chromosome, counted and summed by the size of their aligned part */
                static const uint64_t bin[5] = {1, 100000, 1000000, 5000000, 10000000};
                uint32_t cnt[5] = {0, 0, 0, 0, 0};
                uint64_t sum[5] = {0, 0, 0, 0, 0};
                for (int64_t j = run_first[t]; j < run_first[t + 1]; ++j) {
                    const as_ctg_t *cg = &A.ctg[A.rec[j].ctg];
                    if (cg->chr < 0 || (table == 0) != (cg->chr == t)) continue;
                    for (int b = 0; b < 5; ++b)
                        if (A.rec[j].ta >= bin[b]) {
                            cnt[b]++;
                            sum[b] += A.rec[j].ta;
                        }
                }
                printf("%s\t%d\t%d\t%d\t%d\t%d\t", list[i], (int)cnt[0], (int)cnt[1], (int)cnt[2], (int)cnt[3], (int)cnt[4]);
                pct5(sum, len, '\t');
            } else {
                /* every contig the report puts here that has a PAF record, with the bases it aligns here (kept as uint32), longest first */
                for (int64_t j = run_first[t]; j < run_first[t + 1]; ++j) ta_of[A.rec[j].ctg] = A.rec[j].ta;
                int64_t n = 0;
                for (int64_t q = by_first[t]; q < by_first[t + 1]; ++q)
                    if (A.ctg[by_chr[q]].n_recs > 0) aln[n++] = (uint32_t)ta_of[by_chr[q]];
                for (int64_t j = run_first[t]; j < run_first[t + 1]; ++j) ta_of[A.rec[j].ctg] = 0;
                if (n) qsort(aln, (size_t)n, sizeof(uint32_t), cmp_u32);
                static const double frac[4] = {0.50, 0.90, 0.95, 0.99};
                uint32_t lx[4] = {0, 0, 0, 0};
                uint64_t cov[5] = {0, 0, 0, 0, 0}, s = 0;
                for (int64_t q = 0; q < n; ++q) {
                    const uint32_t a = aln[n - 1 - q];
                    s += a;
                    for (int f = 0; f < 4; ++f)
                        if ((double)s >= (double)len * frac[f] && lx[f] == 0) lx[f] = (uint32_t)(q + 1);
                    for (int f = (int)q; f < 5; ++f) cov[f] += a;
                }
                printf("%s\t%d\t%d\t%d\t%d\t", list[i], (int)lx[0], (int)lx[1], (int)lx[2], (int)lx[3]);
                pct5(cov, len, ',');
            }
        }
    }
    free(ctg_order);
    free(by_first);
    free(by_chr);
    free(run_first);
    free(ta_of);
    free(aln);
    free(A.ctg);
    free(A.chr_len);
    free(A.rec);
    if (!sort_order) free(list);
    recs_free(&ref);
    cli_map_free(&A.ctgs);
    cli_map_free(&A.chrs);
    cli_map_free(&A.names);
    return 0;
}
