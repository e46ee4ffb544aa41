/* qv_main.c — `cornetto qv [-k INT] [-t FILE]... [-c FILE] [-b FILE] [--slots INT] [--accel=no] <truth.fa> <asm.fa> [asm2.fa ...]`, or from reads,
 * `cornetto qv -r reads.fq [-r more.fq] [--min-count INT] [--hist FILE] [--completeness] [--spectra-cn FILE] [...] <asm.fa> [asm2.fa ...]`: the k-mer consensus quality of assemblies
 * against a truth assembly, or against the k-mers that the sample's own accurate reads hold at least --min-count times.  Not in the reference: its
 * protocol (docs/protocol.md:292-303) runs `yak count`
 * and `yak qv` against the HG002 Q100 assembly for asm-1 .. asm-n, primary and hap1+hap2.  The rule is stated once in include/cornetto_accel.h
 * (Merqury's QV from the share of an assembly's k-mers that the truth does not hold; yak's histogram error model is not replicated).
 *
 * The truth files are read once (stream.c) and every batch of their records goes into one set of canonical k-mers that stays resident in HBM
 * (cornetto_kset_add); every assembly is then read the same way and probed against it (cornetto_kset_query).  One device handle serves all files.
 * With -r the set is a counted one (cornetto_kset_open_counted, cornetto_kset_count per batch), its histogram goes to --hist, and the seal with
 * --min-count (cornetto_kset_seal) leaves the plain set that the same probes walk.
 * With --completeness or --spectra-cn every assembly is read once more, in front of the seal while the counts are still there: its k-mers go into
 * the copy counts beside them (cornetto_kset_copies per batch), the spectrum of copies against counts is taken at --min-count
 * (cornetto_kset_spectrum) and the copies are cleared for the next assembly.  The seal drops the k-mers only an assembly held, so the QV pass
 * behind it answers what it answers without the two options.
 * --accel=no / CORNETTO_ACCEL=no: the same rule on the host, a single-threaded open-addressing set (kmer.h has the counted one) and the sequential
 * reader; the same bytes. */
#include <errno.h>
#include <getopt.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "cli.h"
#include "kmer.h"

typedef struct {
    int k;
    int64_t slots;
    /* the truth */
    int64_t t_recs, t_bases;
    cornetto_kset_t *set;                 /* device path */
    uint64_t *tab;                        /* host path: open addressing, linear probing, ~0 = empty */
    int64_t h_pos, h_distinct;
    int reads;                            /* -r: the truth is counted, not inserted */
    cli_kcount_t kc;                      /* host path with -r: the counted table; its key array becomes `tab` at the seal */
    int64_t *x_solid, *x_found;           /* --completeness / --spectra-cn: per assembly, from the pass in front of the seal */
    /* the assembly being read */
    int64_t contigs, bases, kmers, missing;
    FILE *fc, *fb;
} qv_t;

static void qv_overflow(const qv_t *Q)
{
    CLI_ERROR("the k-mer table of %lld slots overflowed: the truth holds more distinct %d-mers; give a larger table with --slots", (long long)Q->slots, Q->k);
    exit(EXIT_FAILURE);
}

/* the same in the copies pass of --completeness / --spectra-cn on the host, where the reads fitted: the k-mers only the assembly holds found no slot */
static void qv_copies_overflow(const qv_t *Q)
{
    CLI_ERROR("the k-mer table of %lld slots overflowed: the assembly holds %d-mers the reads do not, and each takes a slot until the seal; give a larger table with --slots",
              (long long)Q->slots, Q->k);
    exit(EXIT_FAILURE);
}

/* error and qv as the tables print them (the rule: include/cornetto_accel.h) */
static void qv_format(int64_t kmers, int64_t missing, int k, char *e_out, char *q_out, size_t cap)
{
    if (kmers == 0) {
        snprintf(e_out, cap, "NA");
        snprintf(q_out, cap, "NA");
    } else if (missing == 0) {
        snprintf(e_out, cap, "0");
        snprintf(q_out, cap, "inf");
    } else {
        const double p = (double)(kmers - missing) / (double)kmers;
        const double e = 1 - pow(p, 1.0 / k);
        snprintf(e_out, cap, "%.3e", e);
        snprintf(q_out, cap, "%.2f", -10 * log10(e));
    }
}

static void contig_row(qv_t *Q, const char *name, size_t name_len, int64_t len, int64_t kmers, int64_t missing)
{
    Q->contigs++;
    Q->bases += len;
    Q->kmers += kmers;
    Q->missing += missing;
    if (!Q->fc) return;
    char e[48], q[48];
    qv_format(kmers, missing, Q->k, e, q, sizeof(e));
    fwrite(name, 1, name_len, Q->fc);
    fprintf(Q->fc, "\t%lld\t%lld\t%lld\t%s\t%s\n", (long long)len, (long long)kmers, (long long)missing, e, q);
}

static void bed_row(qv_t *Q, const char *name, size_t name_len, int64_t start, int64_t finish)
{
    fwrite(name, 1, name_len, Q->fb);
    fprintf(Q->fb, "\t%lld\t%lld\n", (long long)start, (long long)finish);
}

/* ---------------------------------------------------------------- the device path */
static void truth_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    qv_t *Q = (qv_t *)arg;
    Q->t_recs += n;
    for (int64_t i = 0; i < n; ++i) Q->t_bases += r[i].len;
    const int rc = Q->reads ? cornetto_kset_count(h, Q->set, a, 0) : cornetto_kset_add(h, Q->set, a);
    if (rc == CORNETTO_E_NOMEM) qv_overflow(Q);
    cli_accel_check(h, rc, "qv: inserting the truth's k-mers");
}

static void asm_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    qv_t *Q = (qv_t *)arg;
    int64_t *km = (int64_t *)cli_xmalloc(((size_t)n + 1) * 2 * sizeof(int64_t)), *ms = km + n + 1;
    cornetto_ivl_t *rows = NULL;
    int64_t n_rows = 0;
    cli_accel_check(h, cornetto_kset_query(h, Q->set, a, km, ms, Q->fb ? &rows : NULL, Q->fb ? &n_rows : NULL), "qv: probing the assembly's k-mers");
    for (int64_t i = 0; i < n; ++i) contig_row(Q, r[i].name, (size_t)r[i].name_len, r[i].len, km[i], ms[i]);
    for (int64_t i = 0; i < n_rows; ++i) bed_row(Q, r[rows[i].ctg].name, (size_t)r[rows[i].ctg].name_len, rows[i].start, rows[i].finish);
    cornetto_free(rows);
    free(km);
}

static void copies_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    qv_t *Q = (qv_t *)arg;
    (void)r;
    (void)n;
    const int rc = cornetto_kset_copies(h, Q->set, a);
    if (rc == CORNETTO_E_NOMEM) {          /* the library says which: the assembly-only k-mers found no slot, or the byte a slot could not be had */
        CLI_ERROR("%s: size the table with --slots", cornetto_accel_last_error(h));
        exit(EXIT_FAILURE);
    }
    cli_accel_check(h, rc, "qv: counting the assembly's k-mers");
}

/* ---------------------------------------------------------------- the host path: the same rule, one record at a time */
/* 1 new, 0 present, -1 no room */
static int host_insert(qv_t *Q, uint64_t key)
{
    const uint64_t slots = (uint64_t)Q->slots;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (Q->tab[s] == key) return 0;
        if (Q->tab[s] == ~(uint64_t)0) {
            Q->tab[s] = key;
            return 1;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
    return -1;
}

static int host_has(const qv_t *Q, uint64_t key)
{
    const uint64_t slots = (uint64_t)Q->slots;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (Q->tab[s] == key) return 1;
        if (Q->tab[s] == ~(uint64_t)0) return 0;
        s = s + 1 == slots ? 0 : s + 1;
    }
    return 0;
}

/* every position of the record that holds a k-mer: truth != 0 inserts it, else it is counted, looked up and its span joins the rows */
static void host_record(qv_t *Q, const cli_rec_t *rec, int truth)
{
    const int k = Q->k;
    const unsigned char *s = (const unsigned char *)rec->seq.s;
    const int64_t len = (int64_t)rec->seq.l;
    cli_kroll_t R;
    cli_kroll_init(&R, k);
    int64_t kmers = 0, missing = 0, open_start = -1, open_finish = -1;
    for (int64_t e = 0; e < len; ++e) {
        uint64_t key;
        if (!cli_kroll_push(&R, s[e], &key)) continue;
        const int64_t pos = e - (k - 1);
        if (truth && Q->reads) {
            if (cli_kcount_add(&Q->kc, key, 0) < 0) qv_overflow(Q);
            continue;
        }
        if (truth) {
            const int r = host_insert(Q, key);
            if (r < 0) qv_overflow(Q);
            Q->h_pos++;
            Q->h_distinct += r;
            continue;
        }
        ++kmers;
        if (host_has(Q, key)) continue;
        ++missing;
        if (!Q->fb) continue;
        if (open_start >= 0 && pos <= open_finish) {           /* overlapping or book-ended */
            open_finish = pos + k;
        } else {
            if (open_start >= 0) bed_row(Q, rec->name.s, rec->name.l, open_start, open_finish);
            open_start = pos;
            open_finish = pos + k;
        }
    }
    if (truth) {
        Q->t_recs++;
        Q->t_bases += len;
        return;
    }
    /* (the table of contigs is written before the rows of later contigs, the rows of a contig in one piece: both files are in file order) */
    if (open_start >= 0) bed_row(Q, rec->name.s, rec->name.l, open_start, open_finish);
    contig_row(Q, rec->name.s, rec->name.l, len, kmers, missing);
}

static void host_file(qv_t *Q, const char *path, int truth)
{
    cli_fastx_t *fx = cli_fastx_open(path, 1);
    cli_rec_t *r;
    while ((r = cli_fastx_next_checked(fx)) != NULL) host_record(Q, r, truth);
    cli_fastx_close(fx);
}

/* the k-mers of every record of an assembly into the copy counts of the counted table */
static void host_copies_file(qv_t *Q, const char *path)
{
    cli_fastx_t *fx = cli_fastx_open(path, 1);
    cli_rec_t *r;
    while ((r = cli_fastx_next_checked(fx)) != NULL) {
        const unsigned char *s = (const unsigned char *)r->seq.s;
        cli_kroll_t R;
        cli_kroll_init(&R, Q->k);
        for (size_t e = 0; e < r->seq.l; ++e) {
            uint64_t key;
            if (cli_kroll_push(&R, s[e], &key) && cli_kcount_copy(&Q->kc, key) < 0) qv_copies_overflow(Q);
        }
    }
    cli_fastx_close(fx);
}

/* ---------------------------------------------------------------- sizing */
static void sum_lengths(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    (void)h;
    (void)a;
    for (int64_t i = 0; i < n; ++i) *(int64_t *)arg += r[i].len;
}

/* the bytes of a regular file, or -1 for a FIFO or `-`, which can be read only once.  A file that does not exist gets the reference's open error; exit 1 */
static int64_t regular_size(const char *path)
{
    struct stat st;
    if (!strcmp(path, "-")) return -1;
    if (stat(path, &st) != 0) (void)cli_gz_open(path, 1);
    return S_ISREG(st.st_mode) ? (int64_t)st.st_size : -1;
}

/* kmer.h: an upper bound of the positions of a truth file */
int64_t cli_kmer_file_bound(const char *path)
{
    const int64_t size = regular_size(path);
    if (size < 0) return -1;
    FILE *fp = cli_fopen_chk(path, "rb");
    const int c0 = fgetc(fp), c1 = fgetc(fp);
    fclose(fp);
    if (!(c0 == 0x1f && c1 == 0x8b)) return size;
    int64_t sum = 0;
    stream_names(path, 1, sum_lengths, &sum);
    return sum;
}

static void usage(FILE *fp)
{
    fprintf(fp, "Usage: cornetto qv [options] <truth.fasta> <assembly.fasta> [assembly2.fasta ...]\n");
    fprintf(fp, "       cornetto qv [options] -r <reads.fastq> [-r <more.fastq> ...] <assembly.fasta> [assembly2.fasta ...]\n");
    fprintf(fp, "k-mer consensus quality of assemblies against a truth assembly: the share of every assembly's k-mers that the truth\n");
    fprintf(fp, "does not hold, as error rate and QV (Merqury's rule).  FASTA or FASTQ, plain, gzip or BGZF.\n");
    fprintf(fp, "   -k INT                     k-mer length, odd, 11 to 31 [21]\n");
    fprintf(fp, "   -t FILE                    a further truth file, e.g. the other haplotype (may be repeated)\n");
    fprintf(fp, "   -c FILE                    write the per-contig table to FILE (one assembly only)\n");
    fprintf(fp, "   -b FILE                    write the merged spans of the missing k-mers to FILE as BED (one assembly only)\n");
    fprintf(fp, "   -r FILE                    the truth is the k-mers of these reads from --min-count occurrences upward (may be repeated);\n");
    fprintf(fp, "                              every positional argument is then an assembly\n");
    fprintf(fp, "   --min-count INT            with -r: a k-mer counts as true from INT occurrences in the reads, 1 to 65535 [2]\n");
    fprintf(fp, "   --hist FILE                with -r: write the k-mer count histogram, count<TAB>kmers for counts 1 to 1023 (the last line: 1023 and more)\n");
    fprintf(fp, "   --completeness             with -r: three more columns, solid found completeness: the reads' k-mers from --min-count occurrences upward,\n");
    fprintf(fp, "                              those of them the assembly holds, and their share; every assembly is read twice\n");
    fprintf(fp, "   --spectra-cn FILE          with -r: write the copy-number spectrum, count<TAB>cn0..cn5+ for counts 0 to 1023: the k-mers the reads hold\n");
    fprintf(fp, "                              `count` times and the assembly 0, 1, 2, 3, 4 and more than 4 times (one assembly only; it is read twice)\n");
    fprintf(fp, "   --slots INT                slots of the k-mer table, 8 bytes each, 12 with -r [twice the bases of the truth or the reads;\n");
    fprintf(fp, "                              about 1.5 times the expected distinct k-mers is the usual figure]\n");
    fprintf(fp, "   --accel=no                 run on the host\n");
    fprintf(fp, "   -h                         help\n");
}

static void usage_fail(const char *msg)
{
    CLI_ERROR("%s", msg);
    usage(stderr);
    exit(EXIT_FAILURE);
}

int qv_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"help", no_argument, 0, 'h'}, {"slots", required_argument, 0, 1000}, {"accel", required_argument, 0, 1001},
                                       {"min-count", required_argument, 0, 1002}, {"hist", required_argument, 0, 1003}, {"completeness", no_argument, 0, 1004},
                                       {"spectra-cn", required_argument, 0, 1005}, {0, 0, 0, 0}};
    const char *k_arg = "21", *c_arg = NULL, *b_arg = NULL, *slots_arg = NULL, *mc_arg = NULL, *hist_arg = NULL, *spec_arg = NULL;
    int completeness = 0;
    const char **truth_mem = (const char **)cli_xmalloc(2 * ((size_t)argc + 1) * sizeof(char *)), **truth = truth_mem, **reads = truth + argc + 1;
    int n_truth = 1, n_reads = 0, c, li = 0;
    FILE *fp_help = stderr;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:t:r:c:b:h", lo, &li)) >= 0) {
        if (c == 'k') k_arg = optarg;
        else if (c == 't') truth[n_truth++] = optarg;
        else if (c == 'r') reads[n_reads++] = optarg;
        else if (c == 'c') c_arg = optarg;
        else if (c == 'b') b_arg = optarg;
        else if (c == 1000) slots_arg = optarg;
        else if (c == 1002) mc_arg = optarg;
        else if (c == 1003) hist_arg = optarg;
        else if (c == 1004) completeness = 1;
        else if (c == 1005) spec_arg = optarg;
        else if (c == 1001) {
            if (!strcmp(optarg, "no") || !strcmp(optarg, "n")) cli_host_set(1);
            else if (!strcmp(optarg, "yes") || !strcmp(optarg, "y")) cli_host_set(0);
            else usage_fail("option '--accel' only accepts 'yes' or 'no'");
        } else if (c == 'h') fp_help = stdout;
        else exit(EXIT_FAILURE);
    }
    if (fp_help == stdout) {
        usage(stdout);
        exit(EXIT_SUCCESS);
    }
    if (!n_reads && (mc_arg || hist_arg)) usage_fail("--min-count and --hist go with -r: a truth assembly holds every k-mer once");
    if (!n_reads && (completeness || spec_arg)) usage_fail("--completeness and --spectra-cn go with -r: a truth assembly holds every k-mer once");
    if (n_reads && n_truth > 1) usage_fail("-t names a further truth assembly; it does not go with -r");
    if (argc - optind < (n_reads ? 1 : 2)) {
        usage(stderr);
        exit(EXIT_FAILURE);
    }
    /* with -r every positional is an assembly and the files that fill the table are the reads */
    if (n_reads) {
        truth = reads;
        n_truth = n_reads;
    } else {
        truth[0] = argv[optind];
    }
    char **asms = argv + optind + (n_reads ? 0 : 1);
    const int n_asm = argc - optind - (n_reads ? 0 : 1);
    char *end = NULL;
    long long min_count = 2;
    if (mc_arg) {
        errno = 0;
        min_count = strtoll(mc_arg, &end, 10);
        if (*end || end == mc_arg || errno || min_count < 1 || min_count > CORNETTO_KSET_COUNT_CAP) usage_fail("--min-count: a number from 1 to 65535");
    }
    const long long k = strtoll(k_arg, &end, 10);
    if (*end || end == k_arg || k < 11 || k > 31 || !(k & 1)) usage_fail("-k: k is an odd number from 11 to 31");
    if ((c_arg || b_arg) && n_asm != 1) usage_fail("-c and -b take one assembly");
    if (spec_arg && n_asm != 1) usage_fail("--spectra-cn takes one assembly");
    const int extras = completeness || spec_arg;
    for (int i = 0; extras && i < n_asm; ++i)
        if (regular_size(asms[i]) < 0)          /* (not cli_kmer_file_bound(): it would inflate a whole gzip assembly to say so) */
            usage_fail("--completeness and --spectra-cn read an assembly twice: it cannot be a FIFO or `-`");
    long long slots = 0;
    if (slots_arg) {
        errno = 0;
        slots = strtoll(slots_arg, &end, 10);
        if (*end || end == slots_arg || errno || slots < 1) usage_fail("--slots: a number of at least 1");
    } else {
        for (int i = 0; i < n_truth; ++i) {
            const int64_t b = cli_kmer_file_bound(truth[i]);
            if (b < 0) usage_fail(n_reads ? "a reads file that is a FIFO or `-` can be read only once: size the table with --slots"
                                          : "a truth that is a FIFO or `-` can be read only once: size the table with --slots");
            slots += 2 * b;
        }
        if (slots < 1) slots = 1;
    }

    qv_t Q;
    memset(&Q, 0, sizeof(Q));
    Q.k = (int)k;
    Q.slots = (int64_t)slots;
    Q.reads = n_reads > 0;
    const int host = cli_host_mode();
    cornetto_accel_t *h = NULL;
    int64_t stats[3] = {0, 0, 0};
    if (host && Q.reads) {
        if (cli_kcount_init(&Q.kc, Q.slots, 1) != 0) {
            CLI_ERROR("a k-mer table of %lld slots wants %lld bytes: give a smaller one with --slots", slots, slots * 12);
            exit(EXIT_FAILURE);
        }
        for (int i = 0; i < n_truth; ++i) host_file(&Q, truth[i], 1);
        stats[0] = Q.kc.pos;
        stats[1] = Q.kc.distinct;
    } else if (host) {
        Q.tab = (size_t)slots > SIZE_MAX / 8 ? NULL : (uint64_t *)malloc((size_t)slots * 8);
        if (!Q.tab) {
            CLI_ERROR("a k-mer table of %lld slots wants %lld bytes: give a smaller one with --slots", slots, slots * 8);
            exit(EXIT_FAILURE);
        }
        memset(Q.tab, 0xFF, (size_t)slots * 8);
        for (int i = 0; i < n_truth; ++i) host_file(&Q, truth[i], 1);
        stats[0] = Q.h_pos;
        stats[1] = Q.h_distinct;
    } else {
        h = cli_accel_open();
        const int rc = Q.reads ? cornetto_kset_open_counted(h, Q.k, Q.slots, 1, &Q.set) : cornetto_kset_open(h, Q.k, Q.slots, &Q.set);
        if (rc == CORNETTO_E_NOMEM) {
            CLI_ERROR("%s: give a smaller one with --slots", cornetto_accel_last_error(h));
            exit(EXIT_FAILURE);
        }
        cli_accel_check(h, rc, "qv: the k-mer table");
        for (int i = 0; i < n_truth; ++i) stream_records_on(h, truth[i], 1, truth_scan, &Q);
        cornetto_kset_stats(Q.set, stats);
    }
    if (Q.reads) {
        /* the histogram first, then the seal: from here on the table is the plain set of the solid k-mers */
        if (hist_arg) {
            int64_t hist[CORNETTO_KSET_HIST_BINS];
            if (host) cli_kcount_hist(&Q.kc, 0, hist);
            else cli_accel_check(h, cornetto_kset_hist(h, Q.set, 0, hist), "qv: the histogram of the k-mer counts");
            FILE *fh = cli_fopen_chk(hist_arg, "w");
            for (int i = 1; i < CORNETTO_KSET_HIST_BINS; ++i) fprintf(fh, "%d\t%lld\n", i, (long long)hist[i]);
            if (fclose(fh) != 0) {
                CLI_ERROR("%s", "writing the --hist file failed");
                exit(EXIT_FAILURE);
            }
        }
        const int m = (int)min_count;
        const int32_t m32 = (int32_t)min_count;
        int64_t solid = 0;
        if (extras) {
            /* in front of the seal, while the counts are there: per assembly its copies, the spectrum at the threshold, and the copies cleared */
            int64_t *spec = (int64_t *)cli_xmalloc((size_t)CORNETTO_KSET_CN_BINS * CORNETTO_KSET_HIST_BINS * sizeof(int64_t)), totals[2];
            Q.x_solid = (int64_t *)cli_xmalloc(2 * (size_t)n_asm * sizeof(int64_t));
            Q.x_found = Q.x_solid + n_asm;
            for (int i = 0; i < n_asm; ++i) {
                if (host) {
                    host_copies_file(&Q, asms[i]);
                    cli_kcount_spectrum(&Q.kc, 0, m, spec, totals);
                    cli_kcount_copies_clear(&Q.kc);
                } else {
                    stream_records_on(h, asms[i], 1, copies_scan, &Q);
                    cli_accel_check(h, cornetto_kset_spectrum(h, Q.set, 0, m32, spec, totals), "qv: the copy-number spectrum");
                    cli_accel_check(h, cornetto_kset_copies_clear(h, Q.set), "qv: clearing the copy counts");
                }
                Q.x_solid[i] = totals[0];
                Q.x_found[i] = totals[1];
                if (!spec_arg) continue;
                FILE *fs = cli_fopen_chk(spec_arg, "w");
                fprintf(fs, "#count\tcn0\tcn1\tcn2\tcn3\tcn4\tcn5+\n");
                for (int cbin = 0; cbin < CORNETTO_KSET_HIST_BINS; ++cbin) {
                    fprintf(fs, "%d", cbin);
                    for (int a = 0; a < CORNETTO_KSET_CN_BINS; ++a) fprintf(fs, "\t%lld", (long long)spec[a * CORNETTO_KSET_HIST_BINS + cbin]);
                    fputc('\n', fs);
                }
                if (fclose(fs) != 0) {
                    CLI_ERROR("%s", "writing the --spectra-cn file failed");
                    exit(EXIT_FAILURE);
                }
            }
            free(spec);
        }
        if (host) {
            cli_kcount_seal(&Q.kc, &m, &solid);
            Q.tab = Q.kc.tab;
        } else {
            cli_accel_check(h, cornetto_kset_seal(h, Q.set, &m32, &solid), "qv: sealing the k-mer counts");
        }
        fprintf(stderr, "[qv] reads: %lld records, %lld bases, %lld k-mers, %lld distinct, %lld solid (count >= %d), k=%d\n", (long long)Q.t_recs, (long long)Q.t_bases,
                (long long)stats[0], (long long)stats[1], (long long)solid, m, Q.k);
    } else {
        fprintf(stderr, "[qv] truth: %lld records, %lld bases, %lld k-mers, %lld distinct, k=%d\n", (long long)Q.t_recs, (long long)Q.t_bases, (long long)stats[0],
                (long long)stats[1], Q.k);
    }

    Q.fc = c_arg ? cli_fopen_chk(c_arg, "w") : NULL;
    Q.fb = b_arg ? cli_fopen_chk(b_arg, "w") : NULL;
    if (Q.fc) fprintf(Q.fc, "#contig\tlength\tkmers\tmissing\terror\tqv\n");
    printf(completeness ? "#file\tcontigs\tbases\tkmers\tmissing\terror\tqv\tsolid\tfound\tcompleteness\n" : "#file\tcontigs\tbases\tkmers\tmissing\terror\tqv\n");
    for (int i = 0; i < n_asm; ++i) {
        Q.contigs = Q.bases = Q.kmers = Q.missing = 0;
        if (host) host_file(&Q, asms[i], 0);
        else stream_records_on(h, asms[i], 1, asm_scan, &Q);
        char e[48], q[48];
        qv_format(Q.kmers, Q.missing, Q.k, e, q, sizeof(e));
        printf("%s\t%lld\t%lld\t%lld\t%lld\t%s\t%s", asms[i], (long long)Q.contigs, (long long)Q.bases, (long long)Q.kmers, (long long)Q.missing, e, q);
        if (completeness) {
            printf("\t%lld\t%lld\t", (long long)Q.x_solid[i], (long long)Q.x_found[i]);
            if (Q.x_solid[i]) printf("%.6f", (double)Q.x_found[i] / (double)Q.x_solid[i]);
            else printf("NA");
        }
        putchar('\n');
        fflush(stdout);
    }
    if ((Q.fc && fclose(Q.fc) != 0) || (Q.fb && fclose(Q.fb) != 0)) {
        CLI_ERROR("%s", "writing the -c / -b file failed");
        exit(EXIT_FAILURE);
    }
    if (Q.set) cornetto_kset_free(h, Q.set);
    free(Q.tab);
    free(Q.x_solid);
    free(truth_mem);
    return EXIT_SUCCESS;
}
