/* cli.h — shared declarations of the `cornetto` host CLI (C99) on top of the C ABI in
 * include/cornetto_accel.h.  Drop-in for the reference's CLI on the panel-creation path: same
 * sub-command names, option letters, stdout bytes and exit codes (reference: src/main.c:95-152). */
#ifndef CORNETTO_CLI_H
#define CORNETTO_CLI_H

#include <stdint.h>
#include <stdio.h>

#include "cornetto_accel.h"

#define CORNETTO_VERSION "0.2.0" /* src/cornetto.h:40 */

/* ---- logging (format of src/error.h:54-103; stderr text is not part of parity, exit codes are) ---- */
extern int cli_log_level; /* default 4 = LOG_VERB, src/error.c:33 */
#define CLI_ERROR(...)                                                                                       \
    do {                                                                                                     \
        if (cli_log_level >= 1) {                                                                            \
            fprintf(stderr, "[%s::ERROR]\033[1;31m ", __func__);                                             \
            fprintf(stderr, __VA_ARGS__);                                                                    \
            fprintf(stderr, "\033[0m\n At %s:%d\n", __FILE__, __LINE__ - 1);                                 \
        }                                                                                                    \
    } while (0)
#define CLI_WARNING(...)                                                                                     \
    do {                                                                                                     \
        if (cli_log_level >= 2) {                                                                            \
            fprintf(stderr, "[%s::WARNING]\033[1;33m ", __func__);                                           \
            fprintf(stderr, __VA_ARGS__);                                                                    \
            fprintf(stderr, "\033[0m\n At %s:%d\n", __FILE__, __LINE__ - 1);                                 \
        }                                                                                                    \
    } while (0)
#define CLI_VERBOSE(...)                                                                                     \
    do {                                                                                                     \
        if (cli_log_level >= 4) {                                                                            \
            fprintf(stderr, "[INFO] %s: ", __func__);                                                        \
            fprintf(stderr, __VA_ARGS__);                                                                    \
            fprintf(stderr, "\n");                                                                           \
        }                                                                                                    \
    } while (0)

double cli_realtime(void);
double cli_cputime(void);
long cli_peakrss(void);
void *cli_xmalloc(size_t n);
/* order[k] = index of the k-th longest record, ties in input order (one of the two length arrays is NULL) */
void cli_order_by_length_desc(const int64_t *lens64, const int32_t *lens32, int32_t n, int32_t *order);
void *cli_xrealloc(void *p, size_t n);
char *cli_xstrdup(const char *s);

/* Open the accelerator ($CORNETTO_DEVICE, default 0) or print the reason and exit(EXIT_FAILURE): the
 * host path (host_backend.c) is only ever chosen explicitly. */
cornetto_accel_t *cli_accel_open(void);
/* the same, with the HIP initialisation running on a helper thread between _begin() and _end() (while the input is read);
 * _cancel() drops it when no device work turned up */
/* `want` bytes at file offset `off` with up to n_threads pread() threads -> bytes read (short only at the end of the file), -1 on a read error */
int64_t cli_read_at(int fd, char *dst, int64_t want, int64_t off, int *failed);   /* pread(), or a copy out of a kept mapping for a file on tmpfs */
int64_t cli_pread_parallel(int fd, char *dst, int64_t want, int64_t off, int n_threads);
void cli_accel_open_begin(void);
void cli_accel_warm_hint(int what);   /* before cli_accel_open_begin(): CORNETTO_WARM_* to run behind the open, on a handle of its own */
cornetto_accel_t *cli_accel_open_end(void);
void cli_accel_open_cancel(void);
/* print the handle's last error and exit(EXIT_FAILURE) if rc != 0 */
void cli_ref_abort(const char *msg);   /* stderr line + abort(): where the reference dies on an assert */
void cli_accel_check(cornetto_accel_t *h, int rc, const char *what);

/* ---- record lines on stdout: a plain buffer + decimal formatter (printf costs ~200 ns per field; the window lists have
 * millions of lines).  Goes through stdout's FILE, so it may be mixed with printf as long as cli_out_flush() comes first. */
extern char *cli_out_buf;
extern size_t cli_out_n;
#define CLI_OUT_CAP (1u << 22)
void cli_out_flush(void);
static inline void cli_out_room(size_t need)
{
    if (cli_out_n + need > CLI_OUT_CAP) cli_out_flush();
}
static inline void cli_out_bytes(const char *s, size_t n)
{
    if (n > CLI_OUT_CAP / 2) {
        cli_out_flush();
        fwrite(s, 1, n, stdout);
        return;
    }
    cli_out_room(n);
    for (size_t i = 0; i < n; ++i) cli_out_buf[cli_out_n + i] = s[i];
    cli_out_n += n;
}
static inline void cli_out_char(char c)
{
    cli_out_room(1);
    cli_out_buf[cli_out_n++] = c;
}
static inline void cli_out_int(long long v) /* %lld */
{
    char t[24];
    int k = 0;
    unsigned long long u = v < 0 ? 0ULL - (unsigned long long)v : (unsigned long long)v;
    do {
        t[k++] = (char)('0' + u % 10);
        u /= 10;
    } while (u);
    cli_out_room(24);
    if (v < 0) cli_out_buf[cli_out_n++] = '-';
    while (k) cli_out_buf[cli_out_n++] = t[--k];
}

/* ---- FASTA/FASTQ(+gz) records with the framing rules of klib kseq (src/kseq.h:184-224) ---- */
typedef struct {
    char *s;
    size_t l, m;
} cli_str_t;

typedef struct {
    cli_str_t name, comment, seq, qual;   /* NUL-terminated; seq.l = bases */
} cli_rec_t;

typedef struct cli_fastx cli_fastx_t;
extern int cli_dash_is_stdin;                  /* set by sdust_main: "-" = stdin (the other FASTA sub-commands open a file of that name, as the reference does) */
/* gzopen() for reading (a gzFile).  A file that cannot be opened: the reference's F_CHK message and exit(EXIT_FAILURE) if must_open, else NULL */
void *cli_gz_open(const char *path, int must_open);
cli_fastx_t *cli_fastx_open(const char *path, int must_open); /* a reader over cli_gz_open() */
/* a reader over `n` bytes at `prefix` (borrowed: must outlive the reads of them) followed by the rest of the open
 * gzFile `gz` (owned: closed by cli_fastx_close) */
cli_fastx_t *cli_fastx_open_prefixed(void *gz, const void *prefix, size_t n);
void cli_fastx_close(cli_fastx_t *f);          /* frees the record as well */
/* the next record (the reader's own: valid until the next call), NULL at the end of the file or at a truncated quality string */
cli_rec_t *cli_fastx_next(cli_fastx_t *f);
/* the same where the reference's kseq_t holds the length in an int: a record of more than 2^31-1 bases is an error and exit(EXIT_FAILURE) */
cli_rec_t *cli_fastx_next_checked(cli_fastx_t *f);

/* $CORNETTO_DEVICES: ordinals of the GPUs to spread the contigs over (at most CLI_MAX_DEV); returns how many, 0 if unset */
#define CLI_MAX_DEV 64
int cli_device_list(int *devs);

/* a batch of records held in memory for one device pass */
typedef struct {
    char **names;
    uint8_t **seqs;
    int64_t *lens;
    int32_t n, cap;
    int64_t bases;
} cli_batch_t;
void cli_batch_push(cli_batch_t *b, const char *name, const char *seq, int64_t len);
void cli_batch_take(cli_batch_t *b, const char *name, cli_str_t *seq); /* takes seq's buffer over when it is long */
void cli_batch_clear(cli_batch_t *b);
int64_t cli_batch_limit(void); /* $CORNETTO_BATCH_BASES, default 4e9 */
/* every record of `f` (cli_fastx_next_checked; closed here) in batches of cli_batch_limit() bases, each handed to `fn` and cleared after it */
typedef void (*cli_batch_fn)(cli_batch_t *b, void *arg);
void cli_fastx_batches(cli_fastx_t *f, cli_batch_fn fn, void *arg);

/* ---- the FASTA/FASTQ record streamer of the device path (cli/stream.c) ---- */
typedef struct {
    const char *name;   /* not NUL-terminated */
    int32_t name_len;
    int64_t len;
} cli_recname_t;

/* scan the resident sequences `a` (record i of it = r[i]) and print the sub-command's lines */
typedef void (*scan_fn)(cornetto_accel_t *h, const cli_recname_t *r, int64_t n, const cornetto_asm_t *a, void *arg);

/* every record of the FASTA/FASTQ(+gz) file `path`, framed on the device where the text allows it (else by the sequential reader), handed
 * to `scan` in input order, a batch at a time; must_open: a file that cannot be opened is the reference's F_CHK error (exit 1).
 * warm: the entry points `scan` will call (CORNETTO_WARM_*, or 0), warmed up behind the device open when the input is a large assembly */
void stream_records(const char *path, int must_open, scan_fn scan, void *arg, int warm);
/* the same on the caller's open handle `h`, for a sub-command that reads several files in one process (qv, trioeval): what a call allocates (device
 * text, pinned slabs and pieces) is released before it returns */
void stream_records_on(cornetto_accel_t *h, const char *path, int must_open, scan_fn scan, void *arg);
/* the same for callers that need only every record's name and length: `names` is handed a == NULL.  No bases reach the device (the framing
 * runs with seqs == NULL, the sequential reader uploads nothing); one device handle serves every call of the process, and what a call
 * allocates (device text, pinned slabs and pieces, threads) is released before it returns, so it may be called once per file.
 * CORNETTO_ACCEL=no: the sequential reader alone, no device. */
void stream_names(const char *path, int must_open, scan_fn names, void *arg);

/* ---- text tables shared by fixasm, telocontigs and asmstats (cli/tables.c) ---- */
FILE *cli_fopen_chk(const char *path, const char *mode);   /* fopen(), or the reference's F_CHK message and exit(EXIT_FAILURE) */
/* a string -> dense index map (indices in order of insertion) */
typedef struct {
    int32_t *slot;   /* index + 1, 0 = empty */
    size_t cap;      /* power of two */
    size_t n;
    char **keys;     /* by index, NUL-terminated */
    int32_t *klen;
    size_t kcap;
} cli_map_t;
int32_t cli_map_get(const cli_map_t *m, const char *s, size_t n);              /* -1 if absent */
int32_t cli_map_put(cli_map_t *m, const char *s, size_t n, int *added);       /* the index of s, a new one (*added = 1) if absent */
void cli_map_free(cli_map_t *m);
/* one PAF line as src/pafrec.c:43-98 reads it: strtok on "\t\r\n", atoi() fields; fewer than 12 fields is the reference's
 * "Malformed PAF record" exit(EXIT_FAILURE).  rid / tid point into the line, which is modified. */
typedef struct {
    char *rid, *tid;
    int32_t qlen, qs, qe, tlen, ts, te, match, block;
    int8_t strand;
    uint8_t mapq;
    char tp;
} cli_paf_t;
void cli_paf_parse(char *line, cli_paf_t *r);
/* the rows of one haplotype-to-primary PAF as scripts/create-hapnetto.sh:44,50 uses them (columns 1, 6, 8, 9), appended to a growing array
 * (n, cap in rows): column 6 goes through find_ctg (name -> index of the assembly BED, -1: not there — the row is dropped and counted),
 * column 1 becomes an id of this file's own.  Fewer than 9 tab-separated columns, a coordinate that is not a number of 0 .. 2^31-1 or
 * end <= start: one CLI_ERROR line and exit(EXIT_FAILURE).  -> the rows appended */
typedef int32_t (*cli_name_find_fn)(const char *name, void *arg);
int64_t cli_hap_paf_load(const char *path, cli_name_find_fn find_ctg, void *arg, cornetto_hap_row_t **rows, int64_t *n, int64_t *cap, int64_t *n_dropped);
/* a telomere BED (load_telobed of src/telocontigs.c:59-108 and src/asmstats.c:230-290): sscanf("%s\t%ld\t%ld") per line; fewer than three
 * fields, a negative coordinate or start >= end is exit(EXIT_FAILURE).  on_row(contig name, arg) once per row, in file order. */
void cli_telobed_load(const char *path, void (*on_row)(const char *ctg, void *arg), void *arg);
int cli_strnum_cmp(const char *a, const char *b);   /* natural order of src/misc.c:139-171: digit runs compare as numbers, leading zeros skipped */

/* ---- the host path (cli/host_backend.c): plain sequential C99 for every scan, chosen with --accel=no (noboringbits / boringbits, the
 * reference's own switch: src/boringbits_main.c:627-632) or CORNETTO_ACCEL=no (every sub-command) — never by itself ---- */
int cli_host_mode(void);
void cli_host_set(int on);
/* the hits / intervals of record `ctg` are appended to a growing array (n, cap in records) */
void cli_host_telofind(const uint8_t *seq, int64_t len, const char *motif, int32_t ctg, cornetto_hit_t **hits, int64_t *n_hits, int64_t *cap_hits);
int cli_host_sdust(const uint8_t *seq, int64_t len, int T, int W, int32_t ctg, cornetto_ivl_t **ivls, int64_t *n_ivls, int64_t *cap_ivls); /* -1: -w / -t out of range */
/* same contract as cornetto_telowin(); results are malloc memory */
void cli_host_telowin(const cornetto_hit_t *hits, int64_t n_hits, const int32_t *lens, int32_t n_ctg, double thr_adj, cornetto_win_t **wins, int64_t *n_wins);
/* the rows of cornetto_telo_ends() for ONE record (their ctg = `ctg`), appended to a growing array (n, cap in rows): telofind, telowin, a
 * sequential bedtools merge -d and the intersection with the record's end intervals (scripts/telostats.sh:35-47) */
void cli_host_telo_ends(const uint8_t *seq, int64_t len, const char *motif, double thr_adj, int32_t merge_dist, int32_t ends, int32_t ctg,
                        cornetto_ivl_t **rows, int64_t *n_rows, int64_t *cap_rows);
/* the rows of cornetto_telo_breaks() for ONE record (their ctg = `ctg`), appended to a growing array (n, cap in rows): the host sdust, the
 * host telofind and the interval rule (test/realtest.sh:65-69 on one record); -1: -w / -t out of range */
int cli_host_telo_breaks(const uint8_t *seq, int64_t len, const char *motif, int T, int W, int32_t ctg, cornetto_ivl_t **rows, int64_t *n_rows, int64_t *cap_rows);
/* get_depths(): what the two bedgraphs hold; exits with the reference's messages on malformed input */
typedef struct {
    int32_t n_ctg;
    char **names;
    int32_t *lens;
    int64_t *first;          /* [n_ctg + 1]: contig i is depth[first[i] .. first[i + 1]) */
    uint16_t *depth, *mq;
    int64_t n_pos, n_clamped;
    double sum_depth, sum_mq, positions; /* the reference's double accumulators (:283-285) */
} cli_host_cov_t;
void cli_host_get_depths(FILE *ft, FILE *fq, cli_host_cov_t *out);
/* the same from two RUN-LENGTH bedgraphs (`--runs`, an extension): each file read to its end, the checks of cornetto_bgrun_feed() / _finish()
 * in their order; exits through cli_runs_fail() on malformed input */
void cli_host_get_depths_runs(FILE *ft, FILE *fq, const char *path_t, const char *path_q, cli_host_cov_t *out);
/* the one CLI_ERROR line of a failed check of the run-length readers (kinds of cornetto_bgrunerr_t), then exit(EXIT_FAILURE) */
void cli_runs_fail(const char *path, int kind, long long record, int a, int b);
/* the same from a BAM (`--bam`, an extension): read sequentially through zlib under the rules of cornetto_bamdepth_*() (include/cornetto_accel.h);
 * contigs without positions are left out, as a per-base bedgraph leaves them out; exits through cli_bam_fail() on a malformed file */
void cli_host_get_depths_bam(const char *path, int min_mapq, cli_host_cov_t *out);
/* the one CLI_ERROR line of a failed check of the BAM readers (kinds of cornetto_bamerr_t; 7: no BAM header), then exit(EXIT_FAILURE) */
void cli_bam_fail(const char *path, int kind, long long record, int a, int b);
/* cli/bam.c: the BAM through the device (cornetto_bamdepth_*): the compressed file is read a chunk at a time into one pinned slab, its BGZF chain
 * walked on the host, its blocks fed.  -> 0 with the coverage object (contigs without positions left out) and the malloc'd names; non-zero
 * when a record is larger than the window or the device has no room for the depth arrays: a CLI_WARNING says which, the caller takes the host
 * path; exits through cli_bam_fail() on a malformed file */
int cli_bam_ingest(cornetto_accel_t *h, const char *path, int min_mapq, cornetto_cov_t **cov, int32_t *n_ctg, char ***names, int64_t *n_clamped);
void cli_host_cov_free(cli_host_cov_t *c);
/* `seq --bam` (an extension): the FASTQ text of the BAM's records under the rules of cornetto_bamfq_*() (include/cornetto_accel.h) on stdout, read
 * sequentially through zlib; the first skip_records records are checked and passed over (a caller printed and counted them); stats: reads and
 * bases of both summary lines, added to; exits through cli_bam_fail() on a malformed file, the records in front of the failing one printed */
void cli_host_bam_fastq(const char *path, int min_len, int duplex, int64_t skip_records, uint64_t stats[4]);
/* cli/bam.c: the same through the device (cornetto_bamfq_*), a window of $CORNETTO_BAM_WINDOW bytes at a time, its text pulled in slabs of
 * $CORNETTO_EMIT_SLAB bytes.  -> 0; non-zero when a record is larger than the window (a CLI_WARNING says so): *n_done records are printed and
 * counted in stats, the caller reads the rest on the host */
int cli_bam_fastq(cornetto_accel_t *h, const char *path, int min_len, int duplex, uint64_t stats[4], int64_t *n_done);
/* cli/fasta_cmds.c: the loop of `seq` over the records the sequential reader still has (src/seq.c:116-129): prints the kept ones — through
 * cli_bgzf_out_text() between cli_bgzf_out_begin() and _end() — and adds to stats (reads and bases of both summary lines) */
void cli_seq_records(cli_fastx_t *fx, int min_len, uint64_t stats[4]);
/* cli/fqseq.c: `seq --fastq FILE` (not in the reference): the same text written on the device (cornetto_fqseq_*) from a FASTQ file that is plain,
 * BGZF (inflated on the device) or another gzip; a window of $CORNETTO_FASTQ_WINDOW bytes at a time, its text pulled in slabs of
 * $CORNETTO_EMIT_SLAB bytes.  Where the text stops being plain records, or a record is larger than the window (a CLI_WARNING says so), the
 * sequential reader prints the rest.  stats: added to.  A BGZF file that is not one to its end: cli_bgz_fail(), the text in front printed */
void cli_fastq_seq(cornetto_accel_t *h, const char *path, int min_len, uint64_t stats[4]);
/* cli/qmean.c: `seq -q` (not in the reference; include/cornetto_accel.h states the rule).  seq_main() sets P once (_set; -1: off, the default);
 * every reader of `seq` asks cli_qmean_max_err() for it — the device objects take it through cornetto_*_set_max_err() — and every host loop
 * asks cli_qmean_pass() about the record it is about to print: the n_qual printed quality characters and the n_bases printed bases (true
 * without -q, and for an empty quality line), and counts what it prints with cli_qmean_count(); cli_qmean_add(): what a device object
 * printed.  cli_qmean_printed(): reads and bases of the third summary line. */
void cli_qmean_set(int64_t max_err);
int64_t cli_qmean_max_err(void);
int cli_qmean_pass(const char *qual, size_t n_qual, int64_t n_bases);
void cli_qmean_count(int64_t n_bases);
void cli_qmean_add(int64_t reads, int64_t bases);
void cli_qmean_printed(uint64_t printed[2]);
/* cli/bgzf_out.c: `seq --bam --bgzf` (an extension): between _begin() and _end() the text of both readers above leaves as a BGZF stream on stdout.
 * _text(): text, collected into members of 65280 bytes through zlib; _members(): members the device made (cornetto_bamfq_get_bgzf), behind the
 * pending text; _flush(): the pending text as a member — cli_bam_fail() calls it, so a malformed file leaves the members of the records in front
 * of the failing one; _end(): the same and the 28-byte end-of-file block, on success only */
void cli_bgzf_out_begin(void);
int cli_bgzf_out_active(void);
void cli_bgzf_out_text(const void *p, size_t n);
void cli_bgzf_out_members(const void *p, size_t n);
void cli_bgzf_out_flush(void);
void cli_bgzf_out_end(void);

/* ---- cli/bgcomp.c: compressed depth files of (no)boringbits (mosdepth writes *.per-base.bed.gz, which is BGZF) ---- */
int cli_bgzf_first_member(int fd);   /* is what begins the file a BGZF member? */
/* what a depth file is, by its first bytes: 0 anything that is read as it is (not a regular file: never looked at; or no gzip magic), 1 BGZF, 2 another gzip */
int cli_depth_kind(FILE *fp);
/* The file through zlib on this thread: a FILE * (fopencookie) that hands out the inflated bytes, for the readers that take a FILE *.  kind 1: the BGZF
 * chain is walked block by block (raw inflate, CRC-32 and ISIZE of every footer), kind 2: gzread().  Takes `fp` over (closed with the new one).  What
 * is wrong with the file is one CLI_ERROR line that names it (a BGZF block with its index and offset), then exit(EXIT_FAILURE). */
FILE *cli_zfile_open(const char *path, FILE *fp, int kind);
/* the one CLI_ERROR line of a BGZF file that is not one to its end, then exit(EXIT_FAILURE).  what 0: the block is not what its footer says,
 * 1: what begins there is not a BGZF member, 2: the file ends inside the block */
void cli_bgz_fail(const char *path, int what, long long index, long long offset);
/* A BGZF file for the device readers: pread() threads fill one pinned slab with compressed bytes while the blocks of the other are fed; the chain is
 * walked on the host (cornetto_bgzf_scan), a block cut by the end of a slab opens the next one.  cli_bgz_next(): the next whole blocks that inflate
 * to at most `want` bytes (one block at least) as a source of the cornetto_bg*_feed_src() calls -> their inflated bytes; *last: nothing follows. */
typedef struct cli_bgz cli_bgz_t;
cli_bgz_t *cli_bgz_open(cornetto_accel_t *h, const char *path, int fd, int64_t slab_bytes, int n_rd);
int64_t cli_bgz_next(cornetto_accel_t *h, cli_bgz_t *z, int64_t want, cornetto_bgsrc_t *src, int *last);
void cli_bgz_fail_block(const cli_bgz_t *z, long long index);   /* cli_bgz_fail(.., 0, ..) for block `index` of the file, one of the last source */
void cli_bgz_close(cornetto_accel_t *h, cli_bgz_t *z);
/* get_regs() + the predicate of print_fun_bits (boring = 0) / print_boring_bits (1): the rows to print, malloc memory */
void cli_host_cov_select(const cli_host_cov_t *c, int w, int inc, int32_t lo, int32_t hi, float low_mq, int32_t edge_len, int32_t min_ctg_len, int boring,
                         cornetto_regrec_t **recs, int64_t *n_recs);
void cli_host_merge_windows(const cornetto_regrec_t *recs, int64_t n_recs, int32_t dist, int32_t min_len, cornetto_ivl_t **ivls, int64_t *n_ivls);
/* same contract as cornetto_hap_fun() (rows already checked by cli_hap_paf_load); the result is malloc memory */
void cli_host_hap_fun(const int32_t *ctg_len, int32_t n_ctg, const cornetto_hap_row_t *rows, const int64_t *n_rows, int32_t n_hap, int32_t merge_dist, int32_t flank,
                      cornetto_ivl_t **fun, int64_t *n_fun);
/* same contract as cornetto_telobreaks(); -1: a coordinate outside its contig */
int cli_host_telobreaks(const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *sd, int64_t n_sd, const cornetto_telrow_t *tel, int64_t n_tel,
                        cornetto_ivl_t **out, int64_t *n_out);

/* ---- sub-commands: int xxx_main(int argc, char *argv[]) with argv[0] = sub-command (src/main.c:40-54) ---- */
int depth_main(int argc, char *argv[]);
int boringbits_main(int argc, char *argv[], int8_t boring);
int bigenough_main(int argc, char *argv[]);
int find_telomere_main(int argc, char *argv[]);
int telomere_windows_main(int argc, char *argv[]);
int telomere_breaks_main(int argc, char *argv[]);
int sdust_main(int argc, char *argv[]);
int assbed_main(int argc, char *argv[]);
int seq_main(int argc, char *argv[]);
int fixasm_main(int argc, char *argv[]);
int nx_main(int argc, char *argv[]);
int report_main(int argc, char *argv[]);
int telocontigs_main(int argc, char *argv[]);
int asmstats_main(int argc, char *argv[]);
int telostats_main(int argc, char *argv[]);
int qv_main(int argc, char *argv[]);
int trioeval_main(int argc, char *argv[]);

#endif
