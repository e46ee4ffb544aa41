/* trioeval_main.c — `cornetto trioeval [-k INT] [-P FILE]... [-M FILE]... [-c FILE] [--slots INT] [--accel=no] <pat.fa> <mat.fa> <asm.fa> [asm2.fa ...]`,
 * or from parental reads, `cornetto trioeval --pat-reads FILE [...] --mat-reads FILE [...] [--min-count INT[,INT]] [--hist FILE] [...] <asm.fa> [asm2.fa ...]`:
 * the switch error and the Hamming error of phased assemblies against the k-mers of the two parents.  Not in the reference: its protocol
 * (docs/protocol.md:292-308) runs `yak trioeval pat.yak mat.yak asm.hap1+hap2.fasta` here, from read k-mer counts with thresholds; this works from
 * parental (or truth-haplotype) assemblies, or from parental reads with a count threshold of its own.  The rule is stated once in
 * include/cornetto_accel.h; parity with yak is unpinned.
 *
 * The parental files are read once (stream.c) and every batch of their records goes into one tagged set of canonical k-mers that stays resident
 * in HBM (cornetto_kset_add_tag); every assembly is then read the same way and phased against it (cornetto_kset_phase).  One device handle
 * serves all files.  With parental reads the set is a counted one of two channels (cornetto_kset_open_counted, cornetto_kset_count per batch);
 * its histograms go to --hist, and the seal with --min-count (cornetto_kset_seal) leaves the tagged set that the same phasing walks.
 * --accel=no / CORNETTO_ACCEL=no: the same rule on the host, qv's single-threaded open-addressing set with the tag in the two top bits of a
 * slot (kmer.h has the counted one), and the sequential reader; the same bytes. */
#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>

#include "cli.h"
#include "kmer.h"

#define TRIO_N CORNETTO_TRIO_COUNTS
#define KEYMASK ((((uint64_t)1) << 62) - 1)

typedef struct {
    int k, tag;                           /* tag: of the parental file being read */
    int64_t slots;
    /* the parents */
    int64_t p_recs, p_bases;
    cornetto_kset_t *set;                 /* device path */
    uint64_t *tab;                        /* host path: open addressing, linear probing, key | tag << 62, ~0 = empty */
    int64_t h_pos, h_distinct;
    int reads;                            /* --pat-reads / --mat-reads: the parents are counted, not inserted */
    cli_kcount_t kc;                      /* host path with reads: the counted table; its key array becomes `tab` at the seal */
    /* the assembly being read */
    int64_t contigs, bases, kmers, pat, mat, pairs, switches, hamming;
    FILE *fc;
} trio_t;

static void trio_overflow(const trio_t *T)
{
    CLI_ERROR("the k-mer table of %lld slots overflowed: the parents hold more distinct %d-mers; give a larger table with --slots", (long long)T->slots, T->k);
    exit(EXIT_FAILURE);
}

static void rate_format(int64_t a, int64_t b, char *out, size_t cap)
{
    if (b == 0) snprintf(out, cap, "NA");
    else snprintf(out, cap, "%.6f", (double)a / (double)b);
}

/* c[0 .. 7): kmers, pat, mat, pp, pm, mp, mm of one contig */
static void contig_row(trio_t *T, const char *name, size_t name_len, int64_t len, const int64_t *c)
{
    T->contigs++;
    T->bases += len;
    T->kmers += c[0];
    T->pat += c[1];
    T->mat += c[2];
    T->pairs += c[3] + c[4] + c[5] + c[6];
    T->switches += c[4] + c[5];
    T->hamming += c[1] < c[2] ? c[1] : c[2];
    if (!T->fc) return;
    fwrite(name, 1, name_len, T->fc);
    fprintf(T->fc, "\t%lld", (long long)len);
    for (int i = 0; i < TRIO_N; ++i) fprintf(T->fc, "\t%lld", (long long)c[i]);
    fputc('\n', T->fc);
}

/* ---------------------------------------------------------------- the device path */
static void parent_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    trio_t *T = (trio_t *)arg;
    T->p_recs += n;
    for (int64_t i = 0; i < n; ++i) T->p_bases += r[i].len;
    const int rc = T->reads ? cornetto_kset_count(h, T->set, a, T->tag - 1) : cornetto_kset_add_tag(h, T->set, a, T->tag);
    if (rc == CORNETTO_E_NOMEM) trio_overflow(T);
    cli_accel_check(h, rc, "trioeval: inserting the parents' k-mers");
}

static void asm_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg)
{
    trio_t *T = (trio_t *)arg;
    int64_t *c = (int64_t *)cli_xmalloc(((size_t)n + 1) * TRIO_N * sizeof(int64_t));
    cli_accel_check(h, cornetto_kset_phase(h, T->set, a, c), "trioeval: phasing the assembly's k-mers");
    for (int64_t i = 0; i < n; ++i) contig_row(T, r[i].name, (size_t)r[i].name_len, r[i].len, c + TRIO_N * i);
    free(c);
}

/* ---------------------------------------------------------------- the host path: the same rule, one record at a time */
/* 1 new, 0 present, -1 no room; the tag is OR-ed into the key's slot */
static int host_insert(trio_t *T, uint64_t key, uint64_t tag)
{
    const uint64_t slots = (uint64_t)T->slots;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (T->tab[s] == ~(uint64_t)0) {
            T->tab[s] = key | tag << 62;
            return 1;
        }
        if ((T->tab[s] & KEYMASK) == key) {
            T->tab[s] |= tag << 62;
            return 0;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
    return -1;
}

/* the tag of the key, 0 when it is absent */
static int host_tag(const trio_t *T, uint64_t key)
{
    const uint64_t slots = (uint64_t)T->slots;
    uint64_t s = cli_kmer_mix(key) % slots;
    for (uint64_t step = 0; step < slots; ++step) {
        if (T->tab[s] == ~(uint64_t)0) return 0;
        if ((T->tab[s] & KEYMASK) == key) return (int)(T->tab[s] >> 62);
        s = s + 1 == slots ? 0 : s + 1;
    }
    return 0;
}

/* every position of the record that holds a k-mer: tag != 0 inserts it with the tag, else it is counted, looked up and paired with the marker
 * in front of it */
static void host_record(trio_t *T, const cli_rec_t *rec, int tag)
{
    const unsigned char *s = (const unsigned char *)rec->seq.s;
    const int64_t len = (int64_t)rec->seq.l;
    cli_kroll_t R;
    cli_kroll_init(&R, T->k);
    int64_t c[TRIO_N] = {0};
    int prev = 0;
    for (int64_t e = 0; e < len; ++e) {
        uint64_t key;
        if (!cli_kroll_push(&R, s[e], &key)) continue;
        if (tag && T->reads) {
            if (cli_kcount_add(&T->kc, key, tag - 1) < 0) trio_overflow(T);
            continue;
        }
        if (tag) {
            const int r = host_insert(T, key, (uint64_t)tag);
            if (r < 0) trio_overflow(T);
            T->h_pos++;
            T->h_distinct += r;
            continue;
        }
        c[0]++;
        const int t = host_tag(T, key);
        if (t != CORNETTO_TRIO_PAT && t != CORNETTO_TRIO_MAT) continue;
        c[t]++;
        if (prev) c[3 + (prev - 1) * 2 + (t - 1)]++;
        prev = t;
    }
    if (tag) {
        T->p_recs++;
        T->p_bases += len;
        return;
    }
    contig_row(T, rec->name.s, rec->name.l, len, c);
}

static void host_file(trio_t *T, const char *path, int tag)
{
    cli_fastx_t *fx = cli_fastx_open(path, 1);
    cli_rec_t *r;
    while ((r = cli_fastx_next_checked(fx)) != NULL) host_record(T, r, tag);
    cli_fastx_close(fx);
}

static void usage(FILE *fp)
{
    fprintf(fp, "Usage: cornetto trioeval [options] <pat.fasta> <mat.fasta> <assembly.fasta> [assembly2.fasta ...]\n");
    fprintf(fp, "       cornetto trioeval [options] --pat-reads <pat.fastq> [...] --mat-reads <mat.fastq> [...] <assembly.fasta> [assembly2.fasta ...]\n");
    fprintf(fp, "switch error and Hamming error of phased assemblies against the k-mers of the two parents (or truth haplotypes): a position\n");
    fprintf(fp, "whose k-mer only one parent holds is a marker; a switch is a marker whose type differs from the marker in front of it in\n");
    fprintf(fp, "the contig, the Hamming error of a contig is its minority markers.  FASTA or FASTQ, plain, gzip or BGZF.\n");
    fprintf(fp, "   -k INT                     k-mer length, odd, 11 to 31 [21]\n");
    fprintf(fp, "   -P FILE                    a further paternal file (may be repeated)\n");
    fprintf(fp, "   -M FILE                    a further maternal file (may be repeated)\n");
    fprintf(fp, "   -c FILE                    write the per-contig table to FILE (one assembly only)\n");
    fprintf(fp, "   --pat-reads FILE           the paternal k-mers are those of these reads from --min-count occurrences upward (may be repeated);\n");
    fprintf(fp, "   --mat-reads FILE           the same for the mother; both are needed, and every positional argument is then an assembly\n");
    fprintf(fp, "   --min-count INT[,INT]      with reads: a k-mer counts from INT occurrences, 1 to 65535; one value for both parents or pat,mat [2]\n");
    fprintf(fp, "   --hist FILE                with reads: write the k-mer count histograms, count<TAB>pat<TAB>mat for counts 1 to 1023 (the last line: 1023 and more)\n");
    fprintf(fp, "   --slots INT                slots of the k-mer table, 8 bytes each, 16 with reads [twice the bases of the parents;\n");
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

int trioeval_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"help", no_argument, 0, 'h'}, {"slots", required_argument, 0, 1000}, {"accel", required_argument, 0, 1001},
                                       {"min-count", required_argument, 0, 1002}, {"hist", required_argument, 0, 1003}, {"pat-reads", required_argument, 0, 1004},
                                       {"mat-reads", required_argument, 0, 1005}, {0, 0, 0, 0}};
    const char *k_arg = "21", *c_arg = NULL, *slots_arg = NULL, *mc_arg = NULL, *hist_arg = NULL;
    /* the parental files in reading order: the <pat.fasta> argument, the -P files, <mat.fasta>, the -M files */
    const char **pat_mem = (const char **)cli_xmalloc(4 * ((size_t)argc + 1) * sizeof(char *)), **pat = pat_mem, **mat = pat + argc + 1;
    const char **pat_reads = mat + argc + 1, **mat_reads = pat_reads + argc + 1;
    int n_pat = 1, n_mat = 1, n_pr = 0, n_mr = 0, c, li = 0;
    FILE *fp_help = stderr;
    optind = 1;
    while ((c = getopt_long(argc, argv, "k:P:M:c:h", lo, &li)) >= 0) {
        if (c == 'k') k_arg = optarg;
        else if (c == 'P') pat[n_pat++] = optarg;
        else if (c == 'M') mat[n_mat++] = optarg;
        else if (c == 'c') c_arg = optarg;
        else if (c == 1000) slots_arg = optarg;
        else if (c == 1002) mc_arg = optarg;
        else if (c == 1003) hist_arg = optarg;
        else if (c == 1004) pat_reads[n_pr++] = optarg;
        else if (c == 1005) mat_reads[n_mr++] = optarg;
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
    const int reads = n_pr > 0 || n_mr > 0;
    if (reads && !(n_pr > 0 && n_mr > 0)) usage_fail("--pat-reads and --mat-reads go together: the reads of both parents are needed");
    if (!reads && (mc_arg || hist_arg)) usage_fail("--min-count and --hist go with --pat-reads / --mat-reads: a parental assembly holds every k-mer once");
    if (reads && (n_pat > 1 || n_mat > 1)) usage_fail("-P and -M name further parental assemblies; they do not go with --pat-reads / --mat-reads");
    if (argc - optind < (reads ? 1 : 3)) {
        usage(stderr);
        exit(EXIT_FAILURE);
    }
    /* with parental reads every positional is an assembly and the files that fill the table are the reads */
    if (reads) {
        pat = pat_reads;
        mat = mat_reads;
        n_pat = n_pr;
        n_mat = n_mr;
    } else {
        pat[0] = argv[optind];
        mat[0] = argv[optind + 1];
    }
    char **asms = argv + optind + (reads ? 0 : 2);
    const int n_asm = argc - optind - (reads ? 0 : 2);
    char *end = NULL;
    int min_count[2] = {2, 2};
    if (mc_arg) {
        errno = 0;
        const long long a = strtoll(mc_arg, &end, 10);
        long long b = a;
        const char *second = *end == ',' ? end + 1 : NULL;
        if (end == mc_arg || (*end && !second)) usage_fail("--min-count: one number from 1 to 65535, or two as pat,mat");
        if (second) {
            b = strtoll(second, &end, 10);
            if (*end || end == second) usage_fail("--min-count: one number from 1 to 65535, or two as pat,mat");
        }
        if (errno || a < 1 || a > CORNETTO_KSET_COUNT_CAP || b < 1 || b > CORNETTO_KSET_COUNT_CAP) usage_fail("--min-count: one number from 1 to 65535, or two as pat,mat");
        min_count[0] = (int)a;
        min_count[1] = (int)b;
    }
    const long long k = strtoll(k_arg, &end, 10);
    if (*end || end == k_arg || k < 11 || k > 31 || !(k & 1)) usage_fail("-k: k is an odd number from 11 to 31");
    if (c_arg && n_asm != 1) usage_fail("-c takes one assembly");
    long long slots = 0;
    if (slots_arg) {
        errno = 0;
        slots = strtoll(slots_arg, &end, 10);
        if (*end || end == slots_arg || errno || slots < 1) usage_fail("--slots: a number of at least 1");
    } else {
        for (int i = 0; i < n_pat + n_mat; ++i) {
            const int64_t b = cli_kmer_file_bound(i < n_pat ? pat[i] : mat[i - n_pat]);
            if (b < 0) usage_fail("a parental file that is a FIFO or `-` can be read only once: size the table with --slots");
            slots += 2 * b;
        }
        if (slots < 1) slots = 1;
    }

    trio_t T;
    memset(&T, 0, sizeof(T));
    T.k = (int)k;
    T.slots = (int64_t)slots;
    T.reads = reads;
    const int host = cli_host_mode();
    cornetto_accel_t *h = NULL;
    int64_t stats[3] = {0, 0, 0};
    if (host && reads) {
        if (cli_kcount_init(&T.kc, T.slots, 2) != 0) {
            CLI_ERROR("a k-mer table of %lld slots wants %lld bytes: give a smaller one with --slots", slots, slots * 16);
            exit(EXIT_FAILURE);
        }
    } else if (host) {
        T.tab = (size_t)slots > SIZE_MAX / 8 ? NULL : (uint64_t *)malloc((size_t)slots * 8);
        if (!T.tab) {
            CLI_ERROR("a k-mer table of %lld slots wants %lld bytes: give a smaller one with --slots", slots, slots * 8);
            exit(EXIT_FAILURE);
        }
        memset(T.tab, 0xFF, (size_t)slots * 8);
    } else {
        h = cli_accel_open();
        const int rc = reads ? cornetto_kset_open_counted(h, T.k, T.slots, 2, &T.set) : cornetto_kset_open(h, T.k, T.slots, &T.set);
        if (rc == CORNETTO_E_NOMEM) {
            CLI_ERROR("%s: give a smaller one with --slots", cornetto_accel_last_error(h));
            exit(EXIT_FAILURE);
        }
        cli_accel_check(h, rc, "trioeval: the k-mer table");
    }
    for (int i = 0; i < n_pat + n_mat; ++i) {
        const char *path = i < n_pat ? pat[i] : mat[i - n_pat];
        T.tag = i < n_pat ? CORNETTO_TRIO_PAT : CORNETTO_TRIO_MAT;
        if (host) host_file(&T, path, T.tag);
        else stream_records_on(h, path, 1, parent_scan, &T);
    }
    if (host) {
        stats[0] = reads ? T.kc.pos : T.h_pos;
        stats[1] = reads ? T.kc.distinct : T.h_distinct;
    } else {
        cornetto_kset_stats(T.set, stats);
    }
    if (reads) {
        /* the histograms first, then the seal: from here on the table is the tagged set of the solid k-mers */
        if (hist_arg) {
            int64_t hist[2][CORNETTO_KSET_HIST_BINS];
            for (int ch = 0; ch < 2; ++ch) {
                if (host) cli_kcount_hist(&T.kc, ch, hist[ch]);
                else cli_accel_check(h, cornetto_kset_hist(h, T.set, ch, hist[ch]), "trioeval: the histogram of the k-mer counts");
            }
            FILE *fh = cli_fopen_chk(hist_arg, "w");
            for (int i = 1; i < CORNETTO_KSET_HIST_BINS; ++i) fprintf(fh, "%d\t%lld\t%lld\n", i, (long long)hist[0][i], (long long)hist[1][i]);
            if (fclose(fh) != 0) {
                CLI_ERROR("%s", "writing the --hist file failed");
                exit(EXIT_FAILURE);
            }
        }
        const int32_t m32[2] = {min_count[0], min_count[1]};
        int64_t solid[2] = {0, 0};
        if (host) {
            cli_kcount_seal(&T.kc, min_count, solid);
            T.tab = T.kc.tab;
        } else {
            cli_accel_check(h, cornetto_kset_seal(h, T.set, m32, solid), "trioeval: sealing the k-mer counts");
        }
        fprintf(stderr, "[trioeval] parent reads: %lld records, %lld bases, %lld k-mers, %lld distinct, %lld pat solid, %lld mat solid (count >= %d,%d), k=%d\n",
                (long long)T.p_recs, (long long)T.p_bases, (long long)stats[0], (long long)stats[1], (long long)solid[0], (long long)solid[1], min_count[0], min_count[1], T.k);
    } else {
        fprintf(stderr, "[trioeval] parents: %lld records, %lld bases, %lld k-mers, %lld distinct, k=%d\n", (long long)T.p_recs, (long long)T.p_bases, (long long)stats[0],
                (long long)stats[1], T.k);
    }

    T.fc = c_arg ? cli_fopen_chk(c_arg, "w") : NULL;
    if (T.fc) fprintf(T.fc, "#contig\tlength\tkmers\tpat\tmat\tpp\tpm\tmp\tmm\n");
    printf("#file\tcontigs\tbases\tkmers\tpat\tmat\tpairs\tswitches\tswitch_rate\thamming\thamming_rate\n");
    for (int i = 0; i < n_asm; ++i) {
        T.contigs = T.bases = T.kmers = T.pat = T.mat = T.pairs = T.switches = T.hamming = 0;
        if (host) host_file(&T, asms[i], 0);
        else stream_records_on(h, asms[i], 1, asm_scan, &T);
        char sr[48], hr[48];
        rate_format(T.switches, T.pairs, sr, sizeof(sr));
        rate_format(T.hamming, T.pat + T.mat, hr, sizeof(hr));
        printf("%s\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%s\t%lld\t%s\n", asms[i], (long long)T.contigs, (long long)T.bases, (long long)T.kmers, (long long)T.pat,
               (long long)T.mat, (long long)T.pairs, (long long)T.switches, sr, (long long)T.hamming, hr);
        fflush(stdout);
    }
    if (T.fc && fclose(T.fc) != 0) {
        CLI_ERROR("%s", "writing the -c file failed");
        exit(EXIT_FAILURE);
    }
    if (T.set) cornetto_kset_free(h, T.set);
    free(T.tab);
    free(pat_mem);
    return EXIT_SUCCESS;
}
