/* fasta_cmds.c — the FASTA/FASTQ driven sub-commands: telofind, sdust (device scans), fa2bed, seq (on the host with a positional
 * file, as the reference; `seq --fastq` and `seq --bam` write the same text on the device: cli/fqseq.c, cli/bam.c).
 * Reference: src/find_telomere.c:83-111, src/sdust/sdust.c:179-207, src/assbed.c:50-107,
 * src/seq.c:53-138.  One device: the records come from the streamer (cli/stream.c), one scan per batch, printed in
 * input order.  CORNETTO_DEVICES: the sequential reader's batches are dealt to the devices.  CORNETTO_ACCEL=no: the host path. */
#include <getopt.h>
#include <math.h>
#include <stdlib.h>
#include <pthread.h>
#include <string.h>

#include "cli.h"

static void print_hit(const char *name, size_t name_len, int64_t len, const cornetto_hit_t *h)
{
    cli_out_bytes(name, name_len);   /* "%s\t%zu\t%d\t%zu\t%zu\t%zu\n": src/find_telomere.c:51,56 */
    cli_out_char('\t');
    cli_out_int(len);
    cli_out_char('\t');
    cli_out_int(h->strand);
    cli_out_char('\t');
    cli_out_int(h->start);
    cli_out_char('\t');
    cli_out_int(h->end);
    cli_out_char('\t');
    cli_out_int(h->end - h->start);
    cli_out_char('\n');
}

static void print_ivl(const char *name, size_t name_len, const cornetto_ivl_t *v)
{
    cli_out_bytes(name, name_len);   /* "%s\t%d\t%d\n": src/sdust/sdust.c:201 */
    cli_out_char('\t');
    cli_out_int(v->start);
    cli_out_char('\t');
    cli_out_int(v->finish);
    cli_out_char('\n');
}

/* ---------------------------------------------------------------- telofind */
static void telofind_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n_rec, const cornetto_asm_t *a, void *arg)
{
    (void)n_rec;
    cornetto_hit_t *hits = NULL;
    int64_t n = 0;
    cli_accel_check(h, cornetto_telofind(h, a, (const char *)arg, &hits, &n), "telofind");
    for (int64_t i = 0; i < n; ++i) print_hit(r[hits[i].ctg].name, (size_t)r[hits[i].ctg].name_len, r[hits[i].ctg].len, &hits[i]);
    cli_out_flush();
    cornetto_free(hits);
}

/* ---------------------------------------------------------------- several GPUs of one node
 * CORNETTO_DEVICES=0,1,2,...  (two or more ordinals; a device may be named twice): every scan is independent per record
 * (src/find_telomere.c:101-105, src/sdust/sdust.c:196-203), so the records of a batch are dealt to the devices —
 * longest first, each to the device with the least bases so far (LPT) — and every device gets one host thread with its
 * own handle: upload, scan, results.  Printing happens after the join, record by record in INPUT order (each device's
 * results come back ordered by its local record index, and a device's records keep their input order, so one cursor per
 * device suffices): the output is byte for byte that of one device.  Nothing is exchanged between the devices. */
typedef struct {
    int kind;                    /* 0 telofind, 1 sdust */
    const char *motif;
    int T, W;
} multi_what_t;

typedef struct {
    int dev;
    cornetto_accel_t *h;         /* opened by the worker on its first batch, kept for the next ones */
    const multi_what_t *what;
    const cli_batch_t *b;
    int32_t *mine, n_mine;       /* batch indices of the records of this device, ascending */
    cornetto_hit_t *hits;
    cornetto_ivl_t *ivls;
    int64_t n_res;
    int rc;
    char err[600];
} multi_dev_t;

static void *multi_worker(void *p)
{
    multi_dev_t *d = (multi_dev_t *)p;
    d->rc = CORNETTO_OK;
    d->hits = NULL;
    d->ivls = NULL;
    d->n_res = 0;
    d->err[0] = 0;
    if (!d->h) {
        d->rc = cornetto_accel_open(&d->h, d->dev, NULL);
        if (d->rc != CORNETTO_OK) {
            snprintf(d->err, sizeof(d->err), "cannot open HIP device %d: %s", d->dev, cornetto_accel_strerror(d->rc));
            return NULL;
        }
    }
    if (d->n_mine == 0) return NULL;
    const uint8_t **seqs = (const uint8_t **)cli_xmalloc((size_t)d->n_mine * sizeof(*seqs));
    int64_t *lens = (int64_t *)cli_xmalloc((size_t)d->n_mine * sizeof(*lens));
    for (int32_t i = 0; i < d->n_mine; ++i) {
        seqs[i] = d->b->seqs[d->mine[i]];
        lens[i] = d->b->lens[d->mine[i]];
    }
    cornetto_asm_t *a = NULL;
    d->rc = cornetto_asm_upload(d->h, seqs, lens, d->n_mine, &a);
    if (d->rc == CORNETTO_OK) {
        if (d->what->kind == 0) d->rc = cornetto_telofind(d->h, a, d->what->motif, &d->hits, &d->n_res);
        else d->rc = cornetto_sdust_asm(d->h, a, d->what->T, d->what->W, &d->ivls, &d->n_res);
    }
    if (d->rc != CORNETTO_OK)
        snprintf(d->err, sizeof(d->err), "device %d: %s (%s)", d->dev, cornetto_accel_last_error(d->h), cornetto_accel_strerror(d->rc));
    if (a) cornetto_asm_free(d->h, a);
    free(seqs);
    free(lens);
    return NULL;
}

typedef struct {
    multi_dev_t dv[CLI_MAX_DEV];
    int n_dev;
} multi_t;

static void multi_batch(cli_batch_t *b, void *arg)
{
    multi_t *m = (multi_t *)arg;
    multi_dev_t *dv = m->dv;
    const int n_dev = m->n_dev;
    /* LPT: records by descending length (ties: input order), each to the least loaded device */
    int32_t *order = (int32_t *)cli_xmalloc(((size_t)b->n + 1) * sizeof(*order));
    cli_order_by_length_desc(b->lens, NULL, b->n, order);   /* (a batch may hold hundreds of thousands of reads) */
    int64_t load[CLI_MAX_DEV];
    int32_t *owner = (int32_t *)cli_xmalloc(((size_t)b->n + 1) * sizeof(*owner));
    for (int d = 0; d < n_dev; ++d) { load[d] = 0; dv[d].n_mine = 0; dv[d].b = b; }
    for (int32_t k = 0; k < b->n; ++k) {
        int best = 0;
        for (int d = 1; d < n_dev; ++d)
            if (load[d] < load[best]) best = d;
        owner[order[k]] = best;
        load[best] += b->lens[order[k]] + 1; /* (+1: empty records are spread as well) */
    }
    for (int d = 0; d < n_dev; ++d) dv[d].mine = (int32_t *)cli_xmalloc(((size_t)b->n + 1) * sizeof(int32_t));
    for (int32_t i = 0; i < b->n; ++i) dv[owner[i]].mine[dv[owner[i]].n_mine++] = i; /* ascending = input order */
    pthread_t th[CLI_MAX_DEV];
    int started[CLI_MAX_DEV];
    for (int d = 0; d < n_dev; ++d) started[d] = d > 0 && pthread_create(&th[d], NULL, multi_worker, &dv[d]) == 0;
    for (int d = 0; d < n_dev; ++d)
        if (!started[d]) multi_worker(&dv[d]);
    for (int d = 0; d < n_dev; ++d)
        if (started[d]) pthread_join(th[d], NULL);
    for (int d = 0; d < n_dev; ++d)
        if (dv[d].rc != CORNETTO_OK) {
            CLI_ERROR("%s", dv[d].err);
            exit(EXIT_FAILURE);
        }
    /* input order: record i is local record `local[owner]` of its device; its results are the next ones of that device */
    int64_t cur[CLI_MAX_DEV];
    int32_t local[CLI_MAX_DEV];
    for (int d = 0; d < n_dev; ++d) { cur[d] = 0; local[d] = 0; }
    for (int32_t i = 0; i < b->n; ++i) {
        multi_dev_t *d = &dv[owner[i]];
        const int32_t li = local[owner[i]]++;
        int64_t *c = &cur[owner[i]];
        const size_t nl = strlen(b->names[i]);
        if (d->what->kind == 0)
            for (; *c < d->n_res && d->hits[*c].ctg == li; ++*c) print_hit(b->names[i], nl, b->lens[i], &d->hits[*c]);
        else
            for (; *c < d->n_res && d->ivls[*c].ctg == li; ++*c) print_ivl(b->names[i], nl, &d->ivls[*c]);
    }
    cli_out_flush();
    for (int d = 0; d < n_dev; ++d) {
        cornetto_free(dv[d].hits);
        cornetto_free(dv[d].ivls);
        free(dv[d].mine);
        dv[d].hits = NULL;
        dv[d].ivls = NULL;
    }
    free(order);
    free(owner);
}

/* the whole sub-command over several devices: the sequential reader fills batches, every batch is dealt out */
static void multi_stream(const char *path, int must_open, const multi_what_t *what, const int *devs, int n_dev)
{
    cli_fastx_t *fx = cli_fastx_open(path, must_open);
    if (!fx) return;
    multi_t *m = (multi_t *)cli_xmalloc(sizeof(*m));
    memset(m, 0, sizeof(*m));
    m->n_dev = n_dev;
    for (int d = 0; d < n_dev; ++d) { m->dv[d].dev = devs[d]; m->dv[d].what = what; }
    cli_fastx_batches(fx, multi_batch, m);
    for (int d = 0; d < n_dev; ++d)
        if (m->dv[d].h) cornetto_accel_close(m->dv[d].h);
    free(m);
}

/* the host path (--accel=no / CORNETTO_ACCEL=no): the sequential reader, one record at a time, printed as it is scanned */
static void host_stream(const char *path, int must_open, const multi_what_t *what)
{
    cli_fastx_t *fx = cli_fastx_open(path, must_open);
    if (!fx) return;
    cornetto_hit_t *hits = NULL;
    cornetto_ivl_t *ivls = NULL;
    int64_t n = 0, cap = 0;
    cli_rec_t *r;
    while ((r = cli_fastx_next_checked(fx)) != NULL) {
        const uint8_t *s = (const uint8_t *)r->seq.s;
        const int64_t l = (int64_t)r->seq.l;
        n = 0;
        if (what->kind == 0) {
            cli_host_telofind(s, l, what->motif, 0, &hits, &n, &cap);
            for (int64_t i = 0; i < n; ++i) print_hit(r->name.s, r->name.l, l, &hits[i]);
        } else {
            if (cli_host_sdust(s, l, what->T, what->W, 0, &ivls, &n, &cap) != 0) {
                CLI_ERROR("sdust: -w %d / -t %d outside 3..1026 / 0..2^20", what->W, what->T);
                exit(EXIT_FAILURE);
            }
            for (int64_t i = 0; i < n; ++i) print_ivl(r->name.s, r->name.l, &ivls[i]);
        }
    }
    cli_out_flush();
    free(hits);
    free(ivls);
    cli_fastx_close(fx);
}

int find_telomere_main(int argc, char *argv[])
{
    if (argc < 2) { /* src/find_telomere.c:84-88 */
        fprintf(stderr, "Error: invalid number of parameters\n");
        fprintf(stderr, "Usage: find <input fasta> [optional sequence to search for, default is vertebrate TTAGGG]\n");
        exit(EXIT_FAILURE);
    }
    const char *motif = argc >= 3 ? argv[2] : "TTAGGG";
    if (motif[0] == 0) {
        CLI_ERROR("%s", "empty search sequence");
        exit(EXIT_FAILURE);
    }
    if (cli_host_mode()) {
        const multi_what_t what = {0, motif, 0, 0};
        host_stream(argv[1], 1, &what);
        return EXIT_SUCCESS;
    }
    int devs[CLI_MAX_DEV];
    const int n_dev = cli_device_list(devs);
    if (n_dev >= 2) {
        const multi_what_t what = {0, motif, 0, 0};
        multi_stream(argv[1], 1, &what, devs, n_dev);
        return EXIT_SUCCESS;
    }
    if (n_dev == 1) {
        char one[32];
        snprintf(one, sizeof(one), "%d", devs[0]);
        setenv("CORNETTO_DEVICE", one, 1);
    }
    stream_records(argv[1], 1, telofind_scan, (void *)motif, CORNETTO_WARM_TELO);
    return EXIT_SUCCESS;
}

/* ---------------------------------------------------------------- sdust */
typedef struct {
    int W, T;
} sdust_opt_t;

static void sdust_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n_rec, const cornetto_asm_t *a, void *arg)
{
    (void)n_rec;
    const sdust_opt_t *o = (const sdust_opt_t *)arg;
    cornetto_ivl_t *iv = NULL;
    int64_t n = 0;
    cli_accel_check(h, cornetto_sdust_asm(h, a, o->T, o->W, &iv, &n), "sdust");
    for (int64_t i = 0; i < n; ++i) print_ivl(r[iv[i].ctg].name, (size_t)r[iv[i].ctg].name_len, &iv[i]);
    cli_out_flush();
    cornetto_free(iv);
}

int sdust_main(int argc, char *argv[])
{
    sdust_opt_t o = {64, 20}; /* src/sdust/sdust.c:183 */
    int c;
    cli_dash_is_stdin = 1;    /* src/sdust/sdust.c:194 */
    /* ketopt(..., permute=1, "w:t:") of the reference == POSIX getopt with GNU permutation */
    optind = 1;
    while ((c = getopt(argc, argv, "w:t:")) >= 0) {
        if (c == 'w') o.W = atoi(optarg);
        else if (c == 't') o.T = atoi(optarg);
    }
    if (optind == argc) {
        fprintf(stderr, "Usage: sdust [-w %d] [-t %d] <in.fa>\n", o.W, o.T);
        exit(1);
    }
    if (cli_host_mode()) {
        const multi_what_t what = {1, NULL, o.T, o.W};
        host_stream(argv[optind], 0, &what);
        return 0;
    }
    int devs[CLI_MAX_DEV];
    const int n_dev = cli_device_list(devs);
    if (n_dev >= 2) {
        const multi_what_t what = {1, NULL, o.T, o.W};
        multi_stream(argv[optind], 0, &what, devs, n_dev);
        return 0;
    }
    if (n_dev == 1) {
        char one[32];
        snprintf(one, sizeof(one), "%d", devs[0]);
        setenv("CORNETTO_DEVICE", one, 1);
    }
    stream_records(argv[optind], 0, sdust_scan, &o, CORNETTO_WARM_SDUST);
    return 0;
}

/* ---------------------------------------------------------------- fa2bed */
static const struct option help_only[] = {{"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

int assbed_main(int argc, char *argv[])
{
    FILE *fp_help = stderr;
    int c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "h", help_only, &li)) >= 0)
        if (c == 'h') fp_help = stdout;
    if (argc - optind != 1 || fp_help == stdout) {
        fprintf(fp_help, "Usage: cornetto asmbed <assembly.fasta> \n");
        fprintf(fp_help, "   -h                         help\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    cli_fastx_t *fx = cli_fastx_open(argv[optind], 1);
    cli_rec_t *r;
    while ((r = cli_fastx_next(fx)) != NULL) fprintf(stdout, "%s\t%d\t%d\n", r->name.s, 0, (int)r->seq.l);   /* src/assbed.c:99 */
    cli_fastx_close(fx);
    return 0;
}

/* ---------------------------------------------------------------- seq */
static double seq_min_qscore = 0.0;      /* -q, as it was given: for the third summary line */

static void seq_summary(int min_len, uint64_t before_n, uint64_t before, uint64_t after_n, uint64_t after)
{
    fprintf(stderr, "total reads: %lu\t%lu bases\t%.2f Gbases\n", (unsigned long)before_n, (unsigned long)before, before / 1e9);
    fprintf(stderr, "reads >= %d: %lu\t%lu bases\t%.2f Gbases\n", min_len, (unsigned long)after_n, (unsigned long)after, after / 1e9);
    if (cli_qmean_max_err() >= 0) {      /* -q (not in the reference): the reads that were printed */
        uint64_t p[2];
        cli_qmean_printed(p);
        fprintf(stderr, "mean qscore >= %g: %lu\t%lu bases\t%.2f Gbases\n", seq_min_qscore, (unsigned long)p[0], (unsigned long)p[1], p[1] / 1e9);
    }
}

/* `seq --bam FILE [--duplex] [--bgzf]` (an extension; include/cornetto_accel.h states the rules): a basecaller's BAM to the text `seq` prints */
static int seq_bam(const char *bam, int min_len, int duplex, int bgzf)
{
    uint64_t stats[4] = {0, 0, 0, 0};
    int64_t n_done = 0;
    if (bgzf) cli_bgzf_out_begin();      /* both readers write members from here on; a malformed file exits without the end-of-file block */
    if (!cli_host_mode()) {
        cornetto_accel_t *h = cli_accel_open();
        const int rest = cli_bam_fastq(h, bam, min_len, duplex, stats, &n_done);
        cornetto_accel_close(h);
        if (rest) cli_host_bam_fastq(bam, min_len, duplex, n_done, stats);
    } else {
        cli_host_bam_fastq(bam, min_len, duplex, 0, stats);
    }
    if (bgzf) cli_bgzf_out_end();
    seq_summary(min_len, stats[0], stats[1], stats[2], stats[3]);
    return 0;
}

void cli_seq_records(cli_fastx_t *fx, int min_len, uint64_t stats[4])
{
    const int bgzf = cli_bgzf_out_active();
    cli_rec_t *r;
    while ((r = cli_fastx_next(fx)) != NULL) {
        const int64_t l = (int64_t)r->seq.l;
        stats[1] += (uint64_t)l;
        stats[0]++;
        if (l < min_len) continue;
        stats[3] += (uint64_t)l;
        stats[2]++;
        /* -q: the characters "%s" prints (they end at a byte 0) */
        if (!cli_qmean_pass(r->qual.s, r->qual.l ? strlen(r->qual.s) : 0, (int64_t)strlen(r->seq.s))) continue;
        cli_qmean_count(l);
        if (!bgzf) { /* src/seq.c:120-129: name, TAB, comment */
            printf("@%s", r->name.s);
            if (r->comment.l) printf("\t%s", r->comment.s);
            printf("\n%s\n+\n%s\n", r->seq.s, r->qual.s);
            continue;
        }
        /* the same bytes ("%s" ends at a byte 0) */
        cli_bgzf_out_text("@", 1);
        cli_bgzf_out_text(r->name.s, strlen(r->name.s));
        if (r->comment.l) {
            cli_bgzf_out_text("\t", 1);
            cli_bgzf_out_text(r->comment.s, strlen(r->comment.s));
        }
        cli_bgzf_out_text("\n", 1);
        cli_bgzf_out_text(r->seq.s, strlen(r->seq.s));
        cli_bgzf_out_text("\n+\n", 3);
        cli_bgzf_out_text(r->qual.s, strlen(r->qual.s));
        cli_bgzf_out_text("\n", 1);
    }
}

/* `seq --fastq FILE [--bgzf]` (not in the reference): the text `seq FILE` prints, written on the device; --accel=no: the host loop on FILE */
static int seq_fastq(const char *fastq, int min_len, int bgzf)
{
    uint64_t stats[4] = {0, 0, 0, 0};
    if (bgzf) cli_bgzf_out_begin();      /* a BGZF file that is not one to its end exits without the end-of-file block */
    if (!cli_host_mode()) {
        cornetto_accel_t *h = cli_accel_open();
        cli_fastq_seq(h, fastq, min_len, stats);
        cornetto_accel_close(h);
    } else {
        cli_fastx_t *fx = cli_fastx_open(fastq, 1);
        cli_seq_records(fx, min_len, stats);
        cli_fastx_close(fx);
    }
    if (bgzf) cli_bgzf_out_end();
    seq_summary(min_len, stats[0], stats[1], stats[2], stats[3]);
    return 0;
}

int seq_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"verbose", required_argument, 0, 'v'}, {"min-len", required_argument, 0, 'm'}, {"help", no_argument, 0, 'h'},
                                       {"bam", required_argument, 0, 0}, {"duplex", no_argument, 0, 0}, {"accel", required_argument, 0, 0}, {"bgzf", no_argument, 0, 0},
                                       {"fastq", required_argument, 0, 0}, {"min-qscore", required_argument, 0, 'q'}, {0, 0, 0, 0}};
    FILE *fp_help = stderr;
    int min_len = 30000; /* src/seq.c:63 */
    int c, li = 0, duplex = 0, bgzf = 0;
    const char *bam = NULL, *fastq = NULL;
    optind = 1;
    while ((c = getopt_long(argc, argv, "hm:q:", lo, &li)) >= 0) {
        if (c == 'h') {
            fp_help = stdout;
        } else if (c == 'm') {
            min_len = atoi(optarg);
            if (min_len < 0) {
                fprintf(stderr, "Error: min-len must be a positive integer\n");
                exit(EXIT_FAILURE);
            }
        } else if (c == 'q') {
            char *end = NULL;
            const double t = strtod(optarg, &end);
            if (end == optarg || *end || !(t >= 0.0 && t <= (double)CORNETTO_QUAL_MAX)) {
                fprintf(stderr, "Error: min-qscore must be a number from 0 to %d\n", CORNETTO_QUAL_MAX);
                exit(EXIT_FAILURE);
            }
            seq_min_qscore = t;
            /* the largest mean error probability in units of 10^-9, once, for every path */
            cli_qmean_set((int64_t)floor(1e9 * pow(10.0, -t / 10.0) + 0.5));
        } else if (c == 0 && li == 3) {
            bam = optarg;
        } else if (c == 0 && li == 4) {
            duplex = 1;
        } else if (c == 0 && li == 6) {
            bgzf = 1;
        } else if (c == 0 && li == 7) {
            fastq = optarg;
        } else if (c == 0 && li == 5) {
            if (strcmp(optarg, "no") == 0 || strcmp(optarg, "n") == 0) {
                cli_host_set(1);
            } else if (strcmp(optarg, "yes") == 0 || strcmp(optarg, "y") == 0) {
                cli_host_set(0);
            } else {
                fprintf(stderr, "option '--accel' only accepts 'yes' or 'no'.\n");
            }
        } else {
            fprintf(stderr, "Unknown option: %s\n", argv[optind - 1]);
            exit(EXIT_FAILURE);
        }
    }
    if (fp_help != stdout && bam && argc - optind != 0) {
        CLI_ERROR("%s", "--bam takes the place of the FASTQ file: no positional file with it");
        exit(EXIT_FAILURE);
    }
    if (fp_help != stdout && fastq && bam) {
        CLI_ERROR("%s", "--fastq and --bam each take the place of the FASTQ file: one of them");
        exit(EXIT_FAILURE);
    }
    if (fp_help != stdout && fastq && argc - optind != 0) {
        CLI_ERROR("%s", "--fastq takes the place of the FASTQ file: no positional file with it");
        exit(EXIT_FAILURE);
    }
    if (fp_help != stdout && duplex && !bam) {
        CLI_ERROR("%s", "--duplex: only with --bam (the dx tag is a field of a BAM record)");
        exit(EXIT_FAILURE);
    }
    if (fp_help != stdout && bgzf && !bam && !fastq) {
        CLI_ERROR("%s", "--bgzf: only with --bam or --fastq (the text of a positional FASTQ file is printed as it is)");
        exit(EXIT_FAILURE);
    }
    if ((!bam && !fastq && argc - optind != 1) || fp_help == stdout) {
        fprintf(fp_help, "Usage: cornetto seq <reads.fastq> \n");
        fprintf(fp_help, "   -m INT                     min length [%d]\n", 30000);
        fprintf(fp_help, "   -h                         help\n");
        fprintf(fp_help, "   -q FLOAT                   (not in the reference) --min-qscore: only the reads whose mean error probability is at most 10^(-FLOAT/10)\n");
        fprintf(fp_help, "   --bam FILE                 (extension) the reads of a basecaller's BAM in place of <reads.fastq>, decoded on the device\n");
        fprintf(fp_help, "   --duplex                   (extension) with --bam: only the reads with the tag dx:i:1\n");
        fprintf(fp_help, "   --bgzf                     (not in the reference) with --bam: the text leaves as BGZF, deflated on the device (as bgzip writes it)\n");
        fprintf(fp_help, "   --fastq FILE               (not in the reference) <reads.fastq>, plain or bgzip-compressed, filtered and written on the device\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    if (bam) return seq_bam(bam, min_len, duplex, bgzf);
    if (fastq) return seq_fastq(fastq, min_len, bgzf);
    cli_fastx_t *fx = cli_fastx_open(argv[optind], 1);
    uint64_t stats[4] = {0, 0, 0, 0};
    cli_seq_records(fx, min_len, stats);
    seq_summary(min_len, stats[0], stats[1], stats[2], stats[3]);
    cli_fastx_close(fx);
    return 0;
}
