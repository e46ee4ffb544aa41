/* telostats_main.c — `cornetto telostats [-t 0.4] [-i 99.9] [-e 50000] [-d 100] [-m TTAGGG] [-b out.bed] <asm.fa>`: the reference's
 * scripts/telostats.sh as one sub-command.  The script runs
 *     telofind | awk | telowin 99.9 0.4 | awk | bedtools merge -d 100 | bedtools intersect -wa (contig ends) | sort | uniq -c | awk
 * and writes PREFIX.windows.0.4.50kb.ends.bed, the telomere.bed that telocontigs and asmstats read (scripts/asmstats.sh).  Here the
 * assembly is read once (stream.c), every batch of records goes through cornetto_telo_ends() — nothing but the rows of the BED leaves the
 * device — and stdout is the script's stdout without its first line (`cornetto --version`).  CORNETTO_ACCEL=no: the sequential host path
 * (cli_host_telo_ends), record by record.
 *
 * Where this differs from the script on purpose: the contigs are counted record by record.  The script's `sort | uniq -c` pools two
 * records that carry the same name (bedtools intersect would refuse such an assembly anyway). */
#include <getopt.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "cli.h"

typedef struct {
    const char *motif;
    double thr_adj;
    int32_t merge_dist, ends;
    FILE *bed;
    long long total, one, two, more;
} telostats_t;

/* the rows of a batch (by record index, then by start) -> BED lines and the per-record counts */
static void take_rows(telostats_t *T, const cornetto_ivl_t *rows, int64_t n, const cli_recname_t *r, const char *one_name)
{
    for (int64_t i = 0; i < n;) {
        int64_t k = i;
        while (k < n && rows[k].ctg == rows[i].ctg) ++k;
        for (int64_t q = i; q < k; ++q) {
            if (one_name) fputs(one_name, T->bed);
            else fwrite(r[rows[q].ctg].name, 1, (size_t)r[rows[q].ctg].name_len, T->bed);
            fprintf(T->bed, "\t%d\t%d\n", rows[q].start, rows[q].finish);
        }
        const int64_t c = k - i;                       /* scripts/telostats.sh:56 */
        T->total += c;
        if (c == 1) T->one++;
        else if (c == 2) T->two++;
        else T->more++;
        i = k;
    }
}

static void telostats_scan(cornetto_accel_t *h, const cli_recname_t *r, int64_t n_rec, const cornetto_asm_t *a, void *arg)
{
    (void)n_rec;
    telostats_t *T = (telostats_t *)arg;
    cornetto_ivl_t *rows = NULL;
    int64_t n = 0;
    cli_accel_check(h, cornetto_telo_ends(h, a, T->motif, T->thr_adj, T->merge_dist, T->ends, &rows, &n), "telostats");
    take_rows(T, rows, n, r, NULL);
    cornetto_free(rows);
}

static void usage(FILE *fp)
{
    fprintf(fp, "Usage: cornetto telostats [options] <assembly.fasta>\n");
    fprintf(fp, "Telomere regions at the ends of the contigs (scripts/telostats.sh): telofind, telowin, bedtools merge and\n");
    fprintf(fp, "bedtools intersect against the contig ends in one pass; writes the telomere.bed of telocontigs and asmstats.\n");
    fprintf(fp, "   -t FLOAT                   telowin threshold [0.4]\n");
    fprintf(fp, "   -i FLOAT                   telowin identity in percent [99.9]\n");
    fprintf(fp, "   -e INT                     bases at either end of a contig that count as its ends [50000]\n");
    fprintf(fp, "   -d INT                     merge windows at most INT bases apart, 0 to %d [100]\n", CORNETTO_TELO_ENDS_MAX_DIST);
    fprintf(fp, "   -m STR                     telomere motif [TTAGGG]\n");
    fprintf(fp, "   -b FILE                    write the BED to FILE [PREFIX.windows.<-t>.<-e / 1000>kb.ends.bed]\n");
    fprintf(fp, "   -h                         help\n");
    fprintf(fp, "Contigs are counted record by record: two records of the same name are not pooled (the script's sort | uniq -c\n");
    fprintf(fp, "would pool them, and bedtools rejects such an assembly).\n");
}

int telostats_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    const char *t_arg = "0.4", *i_arg = "99.9", *e_arg = "50000", *d_arg = "100", *motif = "TTAGGG", *bed_arg = NULL;
    FILE *fp_help = stderr;
    int c, li = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "t:i:e:d:m:b:h", lo, &li)) >= 0) {
        if (c == 't') t_arg = optarg;
        else if (c == 'i') i_arg = optarg;
        else if (c == 'e') e_arg = optarg;
        else if (c == 'd') d_arg = optarg;
        else if (c == 'm') motif = optarg;
        else if (c == 'b') bed_arg = optarg;
        else if (c == 'h') fp_help = stdout;
        else exit(EXIT_FAILURE);
    }
    if (argc - optind != 1 || fp_help == stdout) {
        usage(fp_help);
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    const char *file = argv[optind];
    char *end = NULL;
    const double threshold = atof(t_arg);
    if (!(threshold > 0)) {                            /* (NaN as well) no window could fail such a threshold */
        CLI_ERROR("-t %s: the threshold must be greater than 0", t_arg);
        exit(EXIT_FAILURE);
    }
    const long long ends = strtoll(e_arg, &end, 10);
    if (*end || end == e_arg || ends < 1 || ends > 0x7fffffffLL) {
        CLI_ERROR("-e %s: the ends are 1 to 2147483647 bases", e_arg);
        exit(EXIT_FAILURE);
    }
    const long long dist = strtoll(d_arg, &end, 10);
    if (*end || end == d_arg || dist < 0 || dist > CORNETTO_TELO_ENDS_MAX_DIST) {
        CLI_ERROR("-d %s: merge distances of 0 to %d are supported", d_arg, CORNETTO_TELO_ENDS_MAX_DIST);
        exit(EXIT_FAILURE);
    }
    if (motif[0] == 0) {
        CLI_ERROR("%s", "empty search sequence");
        exit(EXIT_FAILURE);
    }
    if (access(file, R_OK) != 0) (void)cli_gz_open(file, 1);   /* scripts/telostats.sh:19, with the words of the reference's open error; exit 1 */

    /* PREFIX = basename FILE .fa, then .fasta (scripts/telostats.sh:20-21) */
    const char *base = strrchr(file, '/');
    char *prefix = cli_xstrdup(base ? base + 1 : file);
    const char *sfx[2] = {".fa", ".fasta"};
    for (int k = 0; k < 2; ++k) {
        const size_t lp = strlen(prefix), ls = strlen(sfx[k]);
        if (lp > ls && !strcmp(prefix + lp - ls, sfx[k])) prefix[lp - ls] = 0;   /* (basename keeps a name that IS the suffix) */
    }
    char *bed_path = NULL;
    if (bed_arg) {
        bed_path = cli_xstrdup(bed_arg);
    } else {                                           /* :23, :46 */
        const size_t cap = strlen(prefix) + strlen(t_arg) + 64;
        bed_path = (char *)cli_xmalloc(cap);
        snprintf(bed_path, cap, "%s.windows.%s.%.0fkb.ends.bed", prefix, t_arg, (double)ends / 1000);
    }

    const double identity = atof(i_arg) / 100;
    telostats_t T = {motif, cornetto_telowin_threshold(threshold, atof(i_arg)), (int32_t)dist, (int32_t)ends, NULL, 0, 0, 0, 0};
    fprintf(stderr, "Given error rate of %.6f running with adjusted threshold of %.6f due to survival prob %.6f\n", identity, T.thr_adj,
            pow(identity, 6));                         /* src/telomere_windows.c:55 */
    printf("genome: %s\nTHRESHOLD: %s\nends: %lld\nasm: %s\n", prefix, t_arg, ends, file);   /* :30-33 */
    printf("Merge telomere motifs in %lldbp\n\n", dist);                                    /* :39-41 */
    printf("Find those at end of scaffolds, within < %lld\n", ends);                         /* :43 */
    fflush(stdout);
    T.bed = cli_fopen_chk(bed_path, "w");

    if (cli_host_mode()) {
        cli_fastx_t *fx = cli_fastx_open(file, 1);
        cornetto_ivl_t *rows = NULL;
        int64_t n = 0, cap = 0;
        cli_rec_t *r;
        while ((r = cli_fastx_next_checked(fx)) != NULL) {
            n = 0;
            cli_host_telo_ends((const uint8_t *)r->seq.s, (int64_t)r->seq.l, motif, T.thr_adj, T.merge_dist, T.ends, 0, &rows, &n, &cap);
            take_rows(&T, rows, n, NULL, r->name.s);
        }
        free(rows);
        cli_fastx_close(fx);
    } else {
        int devs[CLI_MAX_DEV];
        if (cli_device_list(devs) >= 1) {              /* one device: the first one listed */
            char one[32];
            snprintf(one, sizeof(one), "%d", devs[0]);
            setenv("CORNETTO_DEVICE", one, 1);
        }
        stream_records(file, 1, telostats_scan, &T, CORNETTO_WARM_TELO);
    }
    if (fclose(T.bed) != 0) {
        CLI_ERROR("writing %s failed", bed_path);
        exit(EXIT_FAILURE);
    }
    printf("FILE\t%s\n", file);                        /* :51-56 */
    printf("total telomere regions at the end of contigs:\t%lld\n\n\n", T.total);
    printf("contigs with 1 telo:\t%lld\ncontigs with 2 telo:\t%lld\ncontigs with more than 2 telo:\t%lld\n\n", T.one, T.two, T.more);
    free(prefix);
    free(bed_path);
    return EXIT_SUCCESS;
}
