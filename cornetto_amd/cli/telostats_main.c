/* telostats_main.c — `cornetto telostats [-t 0.4] [-i 99.9] [-e 50000] [-d 100] [-m TTAGGG] [-b out.bed] [--breaks FILE] <asm.fa>`: the reference's
 * scripts/telostats.sh as one sub-command.  The script runs
 *     telofind | awk | telowin 99.9 0.4 | awk | bedtools merge -d 100 | bedtools intersect -wa (contig ends) | sort | uniq -c | awk
 * and writes PREFIX.windows.0.4.50kb.ends.bed, the telomere.bed that telocontigs and asmstats read (scripts/asmstats.sh).  Here the
 * assembly is read once (stream.c), every batch of records goes through cornetto_telo_ends() — nothing but the rows of the BED leaves the
 * device — and stdout is the script's stdout without its first line (`cornetto --version`).  CORNETTO_ACCEL=no: the sequential host path
 * (cli_host_telo_ends), record by record.
 *
 * Where this differs from the script on purpose: the contigs are counted record by record.  The script's `sort | uniq -c` pools two
 * records that carry the same name (bedtools intersect would refuse such an assembly anyway).
 *
 * `--breaks FILE`: the telomere breaks of the same pass, the chain of test/realtest.sh:65-69
 *     fa2bed | awk > lens;  sdust > sdust.bed;  telofind > telomere;  telobreaks lens sdust.bed telomere > FILE
 * without its three text files: every batch also goes through cornetto_telo_breaks() (sdust, telofind and the interval rule of
 * csrc/telobreaks_ivl.hip; neither list leaves the device), the few rows of all batches are kept, and after the last batch they are
 * written in the order the chain prints them — contigs in the bucket order of the reference's khash table over the record names in file
 * order (cornetto_khash_str_order), rows by position.  Records that share a name are again taken one by one: their lines come in record
 * order at the place of the name, each with its own length, where the chain would pool them into one bitset of the last length.
 * CORNETTO_ACCEL=no: cli_host_telo_breaks, record by record.  Stdout and the BED do not change with the option. */
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
    /* --breaks: the rows of every batch so far (ctg = index of the record in the file) and every record's name and length */
    int breaks;
    int32_t dust_T, dust_W;
    cornetto_ivl_t *brk;
    int64_t n_brk, cap_brk;
    char **names;
    int32_t *lens;
    int64_t n_rec, cap_rec;
} telostats_t;

static void note_record(telostats_t *T, const char *name, size_t name_len, int64_t len)
{
    if (T->n_rec == T->cap_rec) {
        T->cap_rec = T->cap_rec ? T->cap_rec * 2 : 1024;
        T->names = (char **)cli_xrealloc(T->names, (size_t)T->cap_rec * sizeof(char *));
        T->lens = (int32_t *)cli_xrealloc(T->lens, (size_t)T->cap_rec * sizeof(int32_t));
    }
    if (T->n_rec >= 0x7fffffffLL) {
        CLI_ERROR("%s", "--breaks: more than 2147483647 records");
        exit(EXIT_FAILURE);
    }
    char *nm = (char *)cli_xmalloc(name_len + 1);
    memcpy(nm, name, name_len);
    nm[name_len] = 0;
    T->names[T->n_rec] = nm;
    T->lens[T->n_rec++] = (int32_t)len;
}

/* the break rows of a batch whose first record is record `base` of the file */
static void keep_breaks(telostats_t *T, const cornetto_ivl_t *rows, int64_t n, int64_t base)
{
    if (T->n_brk + n > T->cap_brk) {
        while (T->n_brk + n > T->cap_brk) T->cap_brk = T->cap_brk ? T->cap_brk * 2 : 256;
        T->brk = (cornetto_ivl_t *)cli_xrealloc(T->brk, (size_t)T->cap_brk * sizeof(cornetto_ivl_t));
    }
    for (int64_t i = 0; i < n; ++i) {
        T->brk[T->n_brk] = rows[i];
        T->brk[T->n_brk++].ctg = (int32_t)(base + rows[i].ctg);
    }
}

/* src/telomere_breaks.c:133-148: contigs in khash bucket order, the records of a name in file order, rows by position */
static void write_breaks(const telostats_t *T, FILE *fp)
{
    const int32_t n = (int32_t)T->n_rec;
    int32_t *slot = (int32_t *)cli_xmalloc(((size_t)n + 1) * sizeof(int32_t)), *order = (int32_t *)cli_xmalloc(((size_t)n + 1) * sizeof(int32_t));
    const int32_t n_ids = cornetto_khash_str_order((const char *const *)T->names, n, slot, order);
    if (n_ids < 0) {
        CLI_ERROR("%s", "contig name table failed");
        exit(EXIT_FAILURE);
    }
    /* records by name id (a counting sort keeps file order), rows by record (they are in that order already) */
    int64_t *id_first = (int64_t *)cli_xmalloc(((size_t)n_ids + 2) * sizeof(int64_t)), *row_first = (int64_t *)cli_xmalloc(((size_t)n + 2) * sizeof(int64_t));
    int32_t *by_id = (int32_t *)cli_xmalloc(((size_t)n + 1) * sizeof(int32_t));
    for (int32_t i = 0; i <= n_ids; ++i) id_first[i] = 0;
    for (int32_t i = 0; i < n; ++i) ++id_first[slot[i] + 1];
    for (int32_t i = 0; i < n_ids; ++i) id_first[i + 1] += id_first[i];
    for (int32_t i = 0; i < n; ++i) by_id[id_first[slot[i]]++] = i;
    for (int32_t i = n_ids; i > 0; --i) id_first[i] = id_first[i - 1];
    id_first[0] = 0;
    for (int32_t i = 0; i <= n; ++i) row_first[i] = 0;
    for (int64_t r = 0; r < T->n_brk; ++r) ++row_first[T->brk[r].ctg + 1];
    for (int32_t i = 0; i < n; ++i) row_first[i + 1] += row_first[i];
    for (int32_t k = 0; k < n_ids; ++k)
        for (int64_t q = id_first[order[k]]; q < id_first[order[k] + 1]; ++q) {
            const int32_t rec = by_id[q];
            for (int64_t r = row_first[rec]; r < row_first[rec + 1]; ++r)
                fprintf(fp, "Found telomere positions %d to %d is a telomere in %s of length %d\n", T->brk[r].start, T->brk[r].finish, T->names[rec], T->lens[rec]);   /* :142 */
        }
    free(slot);
    free(order);
    free(id_first);
    free(row_first);
    free(by_id);
}

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
    telostats_t *T = (telostats_t *)arg;
    cornetto_ivl_t *rows = NULL;
    int64_t n = 0;
    cli_accel_check(h, cornetto_telo_ends(h, a, T->motif, T->thr_adj, T->merge_dist, T->ends, &rows, &n), "telostats");
    take_rows(T, rows, n, r, NULL);
    cornetto_free(rows);
    if (!T->breaks) return;
    const int64_t base = T->n_rec;
    for (int64_t i = 0; i < n_rec; ++i) note_record(T, r[i].name, (size_t)r[i].name_len, r[i].len);
    rows = NULL;
    cli_accel_check(h, cornetto_telo_breaks(h, a, T->motif, T->dust_T, T->dust_W, &rows, &n), "telostats --breaks");
    keep_breaks(T, rows, n, base);
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
    fprintf(fp, "   --breaks FILE              also write the telomere breaks to FILE: the lines of sdust + telofind + telobreaks\n");
    fprintf(fp, "   --dust-window INT          sdust window of --breaks, 3 to 1026 [64]\n");
    fprintf(fp, "   --dust-threshold INT       sdust threshold of --breaks, 0 to 1048576 [20]\n");
    fprintf(fp, "   -h                         help\n");
    fprintf(fp, "Contigs are counted record by record: two records of the same name are not pooled (the script's sort | uniq -c\n");
    fprintf(fp, "would pool them, and bedtools rejects such an assembly).  The same holds for --breaks: the lines of such records\n");
    fprintf(fp, "come in record order at the place of the name, each with its own length (telobreaks would pool them into one bitset).\n");
}

int telostats_main(int argc, char *argv[])
{
    static const struct option lo[] = {{"help", no_argument, 0, 'h'}, {"breaks", required_argument, 0, 1000}, {"dust-window", required_argument, 0, 1001},
                                       {"dust-threshold", required_argument, 0, 1002}, {0, 0, 0, 0}};
    const char *t_arg = "0.4", *i_arg = "99.9", *e_arg = "50000", *d_arg = "100", *motif = "TTAGGG", *bed_arg = NULL;
    const char *breaks_arg = NULL, *dw_arg = NULL, *dt_arg = NULL;
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
        else if (c == 1000) breaks_arg = optarg;
        else if (c == 1001) dw_arg = optarg;
        else if (c == 1002) dt_arg = optarg;
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
    if ((dw_arg || dt_arg) && !breaks_arg) {
        CLI_ERROR("%s", "--dust-window / --dust-threshold belong to --breaks");
        exit(EXIT_FAILURE);
    }
    const long long dust_w = dw_arg ? strtoll(dw_arg, &end, 10) : 64;               /* src/sdust/sdust.c:183 */
    if (dw_arg && (*end || end == dw_arg || dust_w < 3 || dust_w > 1026)) {         /* (the limits of cornetto_sdust_asm()) */
        CLI_ERROR("--dust-window %s: windows of 3 to 1026 are supported", dw_arg);
        exit(EXIT_FAILURE);
    }
    const long long dust_t = dt_arg ? strtoll(dt_arg, &end, 10) : 20;
    if (dt_arg && (*end || end == dt_arg || dust_t < 0 || dust_t > (1 << 20))) {
        CLI_ERROR("--dust-threshold %s: thresholds of 0 to 1048576 are supported", dt_arg);
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
    telostats_t T;
    memset(&T, 0, sizeof(T));
    T.motif = motif;
    T.thr_adj = cornetto_telowin_threshold(threshold, atof(i_arg));
    T.merge_dist = (int32_t)dist;
    T.ends = (int32_t)ends;
    T.breaks = breaks_arg != NULL;
    T.dust_T = (int32_t)dust_t;
    T.dust_W = (int32_t)dust_w;
    fprintf(stderr, "Given error rate of %.6f running with adjusted threshold of %.6f due to survival prob %.6f\n", identity, T.thr_adj,
            pow(identity, 6));                         /* src/telomere_windows.c:55 */
    printf("genome: %s\nTHRESHOLD: %s\nends: %lld\nasm: %s\n", prefix, t_arg, ends, file);   /* :30-33 */
    printf("Merge telomere motifs in %lldbp\n\n", dist);                                    /* :39-41 */
    printf("Find those at end of scaffolds, within < %lld\n", ends);                         /* :43 */
    fflush(stdout);
    T.bed = cli_fopen_chk(bed_path, "w");
    FILE *fp_breaks = breaks_arg ? cli_fopen_chk(breaks_arg, "w") : NULL;

    if (cli_host_mode()) {
        cli_fastx_t *fx = cli_fastx_open(file, 1);
        cornetto_ivl_t *rows = NULL;
        int64_t n = 0, cap = 0;
        cli_rec_t *r;
        while ((r = cli_fastx_next_checked(fx)) != NULL) {
            n = 0;
            cli_host_telo_ends((const uint8_t *)r->seq.s, (int64_t)r->seq.l, motif, T.thr_adj, T.merge_dist, T.ends, 0, &rows, &n, &cap);
            take_rows(&T, rows, n, NULL, r->name.s);
            if (!T.breaks) continue;
            n = 0;
            if (cli_host_telo_breaks((const uint8_t *)r->seq.s, (int64_t)r->seq.l, motif, T.dust_T, T.dust_W, 0, &rows, &n, &cap) != 0) {
                CLI_ERROR("--dust-window %d / --dust-threshold %d outside 3..1026 / 0..2^20", T.dust_W, T.dust_T);
                exit(EXIT_FAILURE);
            }
            note_record(&T, r->name.s, r->name.l, (int64_t)r->seq.l);
            keep_breaks(&T, rows, n, T.n_rec - 1);
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
        stream_records(file, 1, telostats_scan, &T, CORNETTO_WARM_TELO | (T.breaks ? CORNETTO_WARM_SDUST : 0));
    }
    if (fclose(T.bed) != 0) {
        CLI_ERROR("writing %s failed", bed_path);
        exit(EXIT_FAILURE);
    }
    if (fp_breaks) {
        write_breaks(&T, fp_breaks);
        if (fclose(fp_breaks) != 0) {
            CLI_ERROR("writing %s failed", breaks_arg);
            exit(EXIT_FAILURE);
        }
    }
    printf("FILE\t%s\n", file);                        /* :51-56 */
    printf("total telomere regions at the end of contigs:\t%lld\n\n\n", T.total);
    printf("contigs with 1 telo:\t%lld\ncontigs with 2 telo:\t%lld\ncontigs with more than 2 telo:\t%lld\n\n", T.one, T.two, T.more);
    free(prefix);
    free(bed_path);
    return EXIT_SUCCESS;
}
