/*
 * cornetto_accel.h — C ABI of libcornetto_hip.so: the MI355X (gfx950) implementation of cornetto's
 * panel-creation hot path.  Plain C, plain pointers and sizes; HIP lives behind it.
 *
 * The reference (hasindu2008/cornetto v0.2.0, paths relative to its root) exposes no FFI: its boundary is
 * the process CLI `cornetto <sub> ...` -> `int xxx_main(int argc, char *argv[])` (src/main.c:40-54,103-134)
 * and, underneath, per-contig C functions.  Each entry point below names the reference unit it replaces.
 * The host CLI in cornetto_amd/cli/ (C99) keeps the sub-command names, option letters, stdout bytes and
 * exit codes and calls only what is declared here.  There is NO CPU fallback behind these symbols: every
 * compute entry point runs HIP kernels and fails with CORNETTO_E_NODEVICE when no GPU is usable.
 *
 * Conventions
 *   - every function returns 0 (CORNETTO_OK) or a negative CORNETTO_E_* status; nothing calls exit()
 *     (the reference's ERROR()+exit(EXIT_FAILURE), src/error.h:97-103, is done by the CLI mains);
 *   - result arrays are allocated by the library (malloc, or pinned host memory from a pool for large
 *     results) and MUST be released with cornetto_free(), never free(); the one exception is
 *     cornetto_sdust(), which keeps the reference's contract (caller free()s);
 *   - calls are synchronous; one cornetto_accel_t may be used by one host thread at a time, and so may one
 *     cornetto_asm_t / cornetto_cov_t: a resident object caches its decomposition tables and the result counts of
 *     its last scan (what the next scan's buffers are sized by), so scans of the same object from two handles must
 *     not run at the same moment (two handles over two objects that wrap the same device memory may);
 *   - coordinates are 0-based, half-open, per contig, 32-bit (kseq_read returns int: src/kseq.h:185).
 */
#ifndef CORNETTO_ACCEL_H
#define CORNETTO_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORNETTO_ACCEL_ABI 1

enum {
    CORNETTO_OK = 0,
    CORNETTO_E_NODEVICE = -1, /* no usable HIP device / HIP runtime error at open */
    CORNETTO_E_HIP = -2,      /* a HIP call or kernel failed; see cornetto_accel_last_error() */
    CORNETTO_E_ARG = -3,      /* invalid argument (NULL, negative length, misaligned device offset, ...) */
    CORNETTO_E_NOMEM = -4,    /* host or device allocation failed */
    CORNETTO_E_UNSUPPORTED = -5, /* parameter outside the implemented range (sdust W > 1026, T > 2^20, ...) */
    CORNETTO_E_FORMAT = -6,      /* malformed input text; see cornetto_bgin_error() */
    CORNETTO_E_ASSERT = -7       /* the reference ends with SIGABRT on these inputs: an assert of get_regs() fails (src/boringbits_main.c:353,368);
                                    cornetto_accel_last_error() names it.  A drop-in caller prints that and abort()s */
};

typedef struct cornetto_accel cornetto_accel_t; /* device + stream + workspaces */
typedef struct cornetto_asm cornetto_asm_t;     /* a set of contigs (or reads) resident in HBM, 1 B/base */
typedef struct cornetto_cov cornetto_cov_t;     /* per-base depth + mq-depth (uint16) of a set of contigs in HBM */

/* one telofind run; replaces one output line of find(): src/find_telomere.c:51,56 */
typedef struct {
    int32_t ctg;    /* index of the contig in the cornetto_asm_t */
    int32_t strand; /* 0 = motif, 1 = reverse complement of the motif */
    int32_t start, end;
} cornetto_hit_t;

/* one telowin window that met the threshold; replaces one printf of process_scaffold():
 * src/telomere_windows.c:37-38.  ratio printed by the caller as (double)car/(end-start), "%.3g". */
typedef struct {
    int32_t ctg;
    int32_t start, end; /* end = start + den */
    int32_t car;        /* marked bases in the window */
} cornetto_win_t;

/* one masked interval of sdust for a set of contigs */
typedef struct {
    int32_t ctg;
    int32_t start, finish;
} cornetto_ivl_t;

/* a coverage window; = reg_t of src/boringbits_main.c:133-138 */
typedef struct {
    int32_t st, end, depth, mq_depth;
} cornetto_reg_t;

/* a selected coverage window of a set of contigs (one stdout line of print_fun_bits / print_boring_bits) */
typedef struct {
    int32_t ctg;
    int32_t st, end, depth, mq_depth;
} cornetto_regrec_t;

/* ---------------------------------------------------------------------------------------------------
 * runtime
 * ------------------------------------------------------------------------------------------------- */

/* number of visible HIP devices (0 when there is none or the runtime is unusable) */
int cornetto_accel_device_count(void);

/* Open device `device` (ordinal among the visible devices).  `stream` is a hipStream_t to launch on, or
 * NULL for a stream owned by the handle.  The seam the reference left for this is --accel=yes|no /
 * CORNETTO_ACC: src/cornetto.h:47, src/boringbits_main.c:627-632. */
int cornetto_accel_open(cornetto_accel_t **h, int device, void *stream);
void cornetto_accel_close(cornetto_accel_t *h);

/* message of the last failure on this handle ("" if none); valid until the next call on the handle */
const char *cornetto_accel_last_error(const cornetto_accel_t *h);
const char *cornetto_accel_strerror(int status);

/* release a result array returned by this library */
void cornetto_free(void *p);

/* Device time of the kernels of the most recent compute call on this handle, measured with HIP events on
 * the handle's stream.  Fills up to `cap` entries of names[]/ms[] (names are static strings) and returns
 * the number of kernels recorded.  Used by bench.py for the live roofline figure. */
int cornetto_accel_last_timing(const cornetto_accel_t *h, const char **names, float *ms, int cap);

/* Share of every compute unit (wave slots and LDS), in percent (10..100, default 100), that the long-running
 * sdust kernel of this handle may occupy.  Lower it when another handle / stream computes on the same device at
 * the same time (bench.py runs telofind and the coverage windows beside sdust): the sdust waves stay resident
 * until their work queue is empty, so what they do not leave free is not available to anybody else meanwhile.
 * Scheduling only: results do not depend on it. */
int cornetto_accel_set_share(cornetto_accel_t *h, int percent);

/* Every entry point of the named groups once on a 4 kb built-in input: what the first use of the runtime costs in a process (loading the code objects,
 * setting the copy engines up, the first pinned pools: 13 of the 25 ms by which the first pass over an assembly exceeded the second) is paid here instead
 * of in the first scan.  Optional; a caller that reads its input first runs it beside that, on the thread that opened the handle.  Nothing the reference
 * has a counterpart for: its per-contig functions start at once (src/sdust/sdust.c:196-203). */
#define CORNETTO_WARM_SDUST 1
#define CORNETTO_WARM_TELO 2
#define CORNETTO_WARM_COV 4
#define CORNETTO_WARM_ALL 7
int cornetto_accel_warm(cornetto_accel_t *h, int what);

/* "The rest of the device is free now" (on != 0) / "is in use again" (on == 0): may be called from ANOTHER host thread than the one that is
 * inside cornetto_sdust_asm() on this handle.  While it is on, a running sdust call whose share is below 100 launches the waves it had left
 * to the other stream as a second kernel that draws from the same chunk counters, and later calls start with the whole chip.  bench.py
 * switches it on when the telofind + coverage thread of a step is through and off when the next step begins.  Scheduling only. */
int cornetto_accel_boost(cornetto_accel_t *h, int on);

/* How many times a cornetto_sdust_asm() call on this handle has put its resident waves on the device so far (readable from any thread while the
 * call runs).  Where the resident waves land decides how much room the other handle's kernels find on every CU for the rest of the call: a caller
 * that starts both sides of a step at once should let the count move before it launches the other side's first kernel — measured on the 3.16 Gbp
 * bench step: 8.2 ms when the sdust waves are there first, 9.2 ms when they arrive 30 us behind the other stream's first kernel. */
unsigned long long cornetto_accel_launch_count(const cornetto_accel_t *h);

/* Lazy result copies (off by default).  While on, cornetto_telo_scan() / cornetto_telofind() and cornetto_cov_select*() return as soon as their
 * kernels are through; the device-to-host copy of the large result array (telomere runs; selected windows) is still in flight on a stream of its
 * own, beside whatever the caller launches next on this handle.  The returned pointers are valid at once, their CONTENT after
 * cornetto_accel_wait().  Wait before reading, before cornetto_free() of such an array and before calling the same entry point again on the
 * handle (its device staging is reused).  Counts and every small output are final when the call returns. */
int cornetto_accel_set_lazy(cornetto_accel_t *h, int on);
int cornetto_accel_wait(cornetto_accel_t *h);

/* Statistics of the production sdust kernel (development / bench aid).  `enable` != 0 makes the following
 * cornetto_sdust_asm() calls on this handle run the counting build of the kernel (a few percent slower); `out`, if not
 * NULL, receives up to `cap` (<= 256) counters of the most recent such call: [2] wave steps, [3] find_perfect calls,
 * [4] groups of 4 steps that took the ungated path, [5] sum and [6] maximum over the waves of their run time in 10 ns ticks, [7] chunks sampled as low-complexity,
 * [10] find_perfect calls with candidates, [11] queue fetch rounds, [12] ticks spent fetching, [16 + 4b ...] per 0.5 ms bin b
 * of wave run time: waves, find_perfect calls with candidates, jobs, find_perfect calls; [254] waves launched, [255] chunks.
 * The sift / resolve kernel (the default for W <= 66) fills instead: [200] resolve steps inside runs of consecutive positions, [201] resolve steps
 * behind a gap (window reads), [202] passes with candidates, [203] positions with more than T / 10 equal words in front, [204] of those after the
 * partial sums over the shortest candidate, [205] after the 16-term sums / the exact walk, [206] tiles of 64 bases, [207] base-by-base steps of
 * chunks with other bytes.
 * Returns the number of counters copied.  Results of sdust do not depend on it. */
int cornetto_accel_sdust_stats(cornetto_accel_t *h, int enable, uint64_t *out, int cap);

/* Which kernel launches are bracketed by HIP events for cornetto_accel_last_timing(): 2 (default) every launch, 1 only
 * the three main kernels (sdust_kernel, cov_blocks, tf_scan), 0 none.  Every event is a packet of its own on the queue;
 * beside a busy second stream the dozen small launches of a call cost about a millisecond more with level 2. */
int cornetto_accel_set_timing(cornetto_accel_t *h, int level);

/* ---------------------------------------------------------------------------------------------------
 * sequences in HBM
 * ------------------------------------------------------------------------------------------------- */

/* Copy n sequences (ASCII, any case, IUPAC allowed, need not be NUL-terminated) to the device.  Replaces
 * the kseq_t.seq buffers the reference scans in place (src/find_telomere.c:101-105, src/sdust/sdust.c:196-199). */
int cornetto_asm_upload(cornetto_accel_t *h, const uint8_t *const *seqs, const int64_t *lens, int32_t n,
                        cornetto_asm_t **out);

/* Wrap bases that already are in device memory: contig i occupies d_bases[offsets[i] .. offsets[i]+lens[i]).
 * Every offset must be a multiple of 64 and the buffer must stay readable for 128 bytes past the last
 * contig (padding content is ignored).  The buffer is borrowed, never freed.  Its CONTENT must not change while the object
 * exists: work decompositions derived from it (chunk / tile tables; with CORNETTO_SDUST_SIFT=0 also the order in which the
 * chunks are handed out, which depends on a sample of the bases) are kept with the object by the first call that needs them.
 * Results stay exact if it does change (the order is a scheduling hint only), the balance of the work does not: wrap again. */
int cornetto_asm_wrap(cornetto_accel_t *h, const void *d_bases, const int64_t *offsets, const int64_t *lens,
                      int32_t n, cornetto_asm_t **out);
void cornetto_asm_free(cornetto_accel_t *h, cornetto_asm_t *a);

/* ---------------------------------------------------------------------------------------------------
 * telofind / telowin
 * ------------------------------------------------------------------------------------------------- */

/* telofind over every contig of `a`: replaces disambiguate()+find() (src/find_telomere.c:76-81,44-74)
 * called per record at :103-104.  motif: any length from 1 byte (up to 32 bytes: the fast path; longer ones are compared
 * byte by byte), compared as the reference does (sequence
 * upper-cased, motif not).  hits come out in the reference's print order: by contig, all strand-0 runs by
 * position, then all strand-1 runs.
 * The hits are placed by 32-bit counts, so an assembly that could hold more than 2^32 - 1 entries of one list is refused
 * by its size alone, whatever it holds (CORNETTO_E_UNSUPPORTED): more than 2^32 - 1 bases for a motif that overlaps a
 * copy of itself or of its reverse complement (AAAA, ACACA) or is longer than 32 bytes, more than about 2^33 bases for
 * any other (bases / 2 + contigs x motif length > 2^32 - 1).  cornetto_telo_scan() with hits has the same limit. */
int cornetto_telofind(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif,
                      cornetto_hit_t **hits, int64_t *n_hits);

/* adjusted threshold of telowin: threshold * pow(identity_percent/100, 6)  (src/telomere_windows.c:53-54) */
double cornetto_telowin_threshold(double threshold, double identity_percent);

/* telowin from explicit hits (what `cornetto telowin in.telomere ...` parses from the TSV): for each of the
 * n_ctg contigs, mark [start,end) of its hits and scan 1000-bp windows, step 200.  Replaces the marking
 * loop + process_scaffold() (src/telomere_windows.c:75-79,28-43).  hits[].ctg indexes ctg_len[]; hits with
 * the same ctg need not be adjacent.  Windows are returned by contig, then by start. */
int cornetto_telowin(cornetto_accel_t *h, const cornetto_hit_t *hits, int64_t n_hits, const int32_t *ctg_len,
                     int32_t n_ctg, double thr_adj, cornetto_win_t **wins, int64_t *n_wins);

/* fused telofind -> telowin on the device (no TSV round trip, the mark bitmap never leaves HBM).
 * Equivalent to cornetto_telofind() followed by cornetto_telowin() on its hits.  hits/n_hits may be NULL. */
int cornetto_telo_scan(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, double thr_adj,
                       cornetto_hit_t **hits, int64_t *n_hits, cornetto_win_t **wins, int64_t *n_wins);

/* The telomere regions at the contig ends, i.e. the rows of PREFIX.windows.0.4.50kb.ends.bed of scripts/telostats.sh:35-47, in one pass
 * on the device:  telofind | telowin (thr_adj = cornetto_telowin_threshold(0.4, 99.9)) | bedtools merge -d merge_dist | bedtools
 * intersect -wa against the end intervals of every contig — [0, ends) and [len - ends, len) if len > 2 ends, else [0, len) (:44).
 * The qualifying windows of a contig (src/telomere_windows.c:31-41) are merged while the next one starts at most merge_dist behind the
 * end of the last; a region is returned once per end interval it overlaps by at least one base (0, 1 or 2 times, the copies adjacent),
 * regions by contig index, then by start.  Neither the hits nor the windows leave the device.  ends >= 1;
 * 0 <= merge_dist <= CORNETTO_TELO_ENDS_MAX_DIST (CORNETTO_E_UNSUPPORTED beyond).  Release rows with cornetto_free(). */
#define CORNETTO_TELO_ENDS_MAX_DIST 11799
int cornetto_telo_ends(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, double thr_adj, int32_t merge_dist, int32_t ends,
                       cornetto_ivl_t **rows, int64_t *n_rows);

/* ---------------------------------------------------------------------------------------------------
 * sdust
 * ------------------------------------------------------------------------------------------------- */

/* symmetric DUST over every contig of `a`; replaces sdust() called per record at src/sdust/sdust.c:199
 * (sdust_core :130-160).  3 <= W <= 1026 (CORNETTO_E_UNSUPPORTED beyond: there the reference's own int products overflow), T >= 0.  Intervals by contig, then by start; per contig they are
 * exactly the reference's (start<<32|finish) list, including intervals that run past the contig end
 * after an N run. */
int cornetto_sdust_asm(cornetto_accel_t *h, const cornetto_asm_t *a, int32_t T, int32_t W,
                       cornetto_ivl_t **ivls, int64_t *n_ivls);

/* The same call in two parts, for a host that has other work for the device meanwhile (a second stream through a second handle) and no thread
 * to spare: _begin queues the call on the handle's stream and returns without waiting WHEN the rest of the call can be sized by the counts the
 * last call over the same assembly, T and W left behind (the scan, the kernel, the stitch and the result copy in one go; the counts are checked
 * by _end, and a call whose counts outgrew them is run again the long way: never a truncated answer); otherwise — the first call for an
 * assembly, the statistics build — it queues nothing (cornetto_accel_launch_count() tells) and _end runs the whole call.  Between the two the
 * handle must not be used for anything else; the same (a, T, W) go to both.  Results, order and errors are those of cornetto_sdust_asm(). */
int cornetto_sdust_asm_begin(cornetto_accel_t *h, const cornetto_asm_t *a, int32_t T, int32_t W);
int cornetto_sdust_asm_end(cornetto_accel_t *h, const cornetto_asm_t *a, int32_t T, int32_t W,
                           cornetto_ivl_t **ivls, int64_t *n_ivls);

/* Drop-in for `uint64_t *sdust(void *km, const uint8_t *seq, int l_seq, int T, int W, int *n)`
 * (src/sdust/sdust.h:19): same arguments, same ownership (caller free()s), l_seq < 0 means strlen.
 * km must be NULL.  Uses a process-wide handle on device $CORNETTO_DEVICE (default 0); returns NULL and
 * sets *n = -1 when the device path is unavailable. */
uint64_t *cornetto_sdust(void *km, const uint8_t *seq, int l_seq, int T, int W, int *n);

/* Drop-ins for the buffered interface of src/sdust/sdust.h:16-21 (`sdust_buf_init`, `sdust_buf_destroy`, `sdust_core`):
 * the result array belongs to the buf, is valid until the next cornetto_sdust_core() on that buf or its destruction, and
 * must not be freed by the caller.  km must be NULL.  Same process-wide handle as cornetto_sdust(); NULL and *n = -1
 * when the device path is unavailable. */
typedef struct cornetto_sdust_buf cornetto_sdust_buf_t;
cornetto_sdust_buf_t *cornetto_sdust_buf_init(void *km);
void cornetto_sdust_buf_destroy(cornetto_sdust_buf_t *buf);
const uint64_t *cornetto_sdust_core(const uint8_t *seq, int l_seq, int T, int W, int *n, cornetto_sdust_buf_t *buf);

/* ---------------------------------------------------------------------------------------------------
 * (no)boringbits window stage
 * ------------------------------------------------------------------------------------------------- */

/* Copy per-base depth arrays of n contigs to the device; replaces ctg_depth_t.depth/.mq_depth filled by
 * get_depths() (src/boringbits_main.c:116-122,279-281). */
int cornetto_cov_upload(cornetto_accel_t *h, const uint16_t *const *depth, const uint16_t *const *mq_depth,
                        const int32_t *lens, int32_t n, cornetto_cov_t **out);

/* Wrap arrays already in device memory; offsets are in ELEMENTS and must be multiples of 64; both arrays
 * must stay readable for 64 elements past the last contig. */
int cornetto_cov_wrap(cornetto_accel_t *h, const void *d_depth, const void *d_mq_depth, const int64_t *offsets,
                      const int32_t *lens, int32_t n, cornetto_cov_t **out);
void cornetto_cov_free(cornetto_accel_t *h, cornetto_cov_t *c);

/* Several GPUs: copy contigs ctgs[0..n) (indices into `src`, any order) of a coverage object that is resident on the device of
 * h_src into a new object on the device of h_dst (the same device is allowed).  get_regs() is independent per contig
 * (src/boringbits_main.c:331); the one quantity that spans contigs is the assembly-wide mean behind the thresholds
 * (:283-294 -> :518-519): every device runs cornetto_cov_prepare() on its share, the caller adds the sums[] up. */
int cornetto_cov_shard(cornetto_accel_t *h_src, const cornetto_cov_t *src, cornetto_accel_t *h_dst, const int32_t *ctgs, int32_t n,
                       cornetto_cov_t **out);

/* number of contigs and their lengths (owned by the object) */
int32_t cornetto_cov_n(const cornetto_cov_t *c);
const int32_t *cornetto_cov_lens(const cornetto_cov_t *c);

/* the two arrays of contig `ctg`, position by position, into caller-provided depth[] and mq_depth[] (cornetto_cov_lens()[ctg] elements
 * each; either may be NULL) */
int cornetto_cov_download(cornetto_accel_t *h, const cornetto_cov_t *c, int32_t ctg, uint16_t *depth, uint16_t *mq_depth);

/* number of windows of a contig: src/boringbits_main.c:338-339 */
int32_t cornetto_n_reg(int32_t length, int32_t window_size, int32_t window_inc);

/* The asserts of get_regs() for one contig (src/boringbits_main.c:353 `st<end`, :368 `end == length`): 0 when the reference computes
 * the windows, else the line of the assert that aborts it.  With 1 <= window_inc <= window_size and length >= 1 always 0; with
 * window_inc > window_size the windows are sparse ([j*inc, min(j*inc + w, length))) and the last one has to reach the contig's end. */
int32_t cornetto_regs_assert(int32_t length, int32_t window_size, int32_t window_inc);

/* Stage 1: per-`window_inc` block sums on the device plus the exact totals the mean needs.
 * sums[0] = sum of depth, sums[1] = sum of mq_depth, sums[2] = number of positions; the caller forms
 * mean = (int)round(sums[0]/sums[2]) (src/boringbits_main.c:283-285,293-294) — across ranks after an
 * all-reduce of sums[].  For a coverage read from bedgraph text that holds NEGATIVE depth values (the reference takes them: %d) the
 * arrays hold their uint16 (:282-283) and the totals the values themselves (:285-286): sums[0] and sums[1] are then two's complement
 * numbers — form the mean from (int64_t)sums[.].  Needs window_inc >= 1; window_inc > window_size is computed as the reference computes it (:346-366).
 * CORNETTO_E_ASSERT when cornetto_regs_assert() is non-zero for any contig: get_regs() runs over EVERY contig before the
 * reference prints anything, so the process ends there with nothing on stdout. */
int cornetto_cov_prepare(cornetto_accel_t *h, cornetto_cov_t *c, int32_t window_size, int32_t window_inc,
                         uint64_t sums[3]);

/* get_regs() for one contig (src/boringbits_main.c:346-366): all cornetto_n_reg() windows, in order, into
 * caller-provided regs[].  cornetto_cov_prepare() must have been called with the same sizes. */
int cornetto_cov_regs(cornetto_accel_t *h, const cornetto_cov_t *c, int32_t ctg, cornetto_reg_t *regs);

/* thresholds: (int)round(factor * mean) with the product formed in float (src/boringbits_main.c:518-519) */
int32_t cornetto_cov_threshold(float factor, int32_t mean);

/* Stage 2: classify every window and return the selected ones in print order (contig, then st).
 *   boring == 0: print_fun_bits  (src/boringbits_main.c:425-445) — windows of contigs with
 *                len >= min_ctg_len that satisfy depth<lo || depth>hi || mq/(double)depth < low_mq;
 *                (the caller prints the '.' edge / short-contig lines, which need no data);
 *   boring != 0: print_boring_bits (:463-481) — contigs with len > min_ctg_len, windows with
 *                st > edge_len && end < len - edge_len that do NOT satisfy the predicate. */
int cornetto_cov_select(cornetto_accel_t *h, const cornetto_cov_t *c, int32_t lo, int32_t hi, float low_mq,
                        int32_t edge_len, int32_t min_ctg_len, int boring, cornetto_regrec_t **recs,
                        int64_t *n_recs);

/* The same selection in packed form, for callers that take millions of windows per call (the whole-assembly panel: 7.5 M
 * windows of a 3 Gbp assembly are 150 MB as cornetto_regrec_t, 60 MB packed): 8 bytes per window, the contig given by
 * position — the windows of contig i are recs[ctg_first[i] .. ctg_first[i + 1]) (ctg_first has n + 1 entries) — and
 * end = min(st + window_size, length of the contig) (src/boringbits_main.c:348-351).  depth and mq_depth are means of uint16
 * values (:354-361), so they fit.  Release recs and ctg_first with cornetto_free(). */
typedef struct {
    int32_t st;
    uint16_t depth, mq_depth;
} cornetto_regpk_t;
int cornetto_cov_select_packed(cornetto_accel_t *h, const cornetto_cov_t *c, int32_t lo, int32_t hi, float low_mq,
                               int32_t edge_len, int32_t min_ctg_len, int boring, cornetto_regpk_t **recs, int64_t *n_recs,
                               int64_t **ctg_first);

/* One pass of the panel path over a resident assembly and its resident coverage in one call: cornetto_cov_prepare() ->
 * cornetto_cov_threshold() x 2 (mean = (int)round(sums[0] / sums[2]), src/boringbits_main.c:293, :518-519) ->
 * cornetto_cov_select_packed() -> cornetto_telo_scan(), the same kernels and the same results.  What it saves is host round trips:
 * everything behind the totals is queued in one go, sized by the counts the previous step over the same objects gave and checked
 * afterwards (two synchronisations instead of five; a count that outgrew its estimate repeats that part through the exact entry
 * point).  `exchange`, if not NULL, is called once with the three sums of THIS process's contigs and replaces them by the sums
 * over all processes (one rank per GPU: a 3 x int64 all-reduce — the one exchange the path has, :283-294 -> :518-519); it returns 0
 * or an error.  sums[] and thr[] (low, high) are returned; result arrays as from the single entry points (cornetto_free / free).
 * With lazy copies (cornetto_accel_set_lazy) the contents of recs / hits are complete after cornetto_accel_wait().
 * window_size above 32768 is CORNETTO_E_UNSUPPORTED here as in cornetto_cov_select_packed() (the packed record's 16-bit means). */
typedef struct {
    const char *motif;              /* telofind motif (src/find_telomere.c:101-105) */
    double thr_adj;                 /* cornetto_telowin_threshold() */
    int32_t window_size, window_inc;
    float low_cov, high_cov, low_mq;   /* -L -H -Q */
    int32_t edge_len, min_ctg_len;     /* -e -m */
    int32_t boring;                    /* 0: noboringbits' selection, 1: the deprecated boringbits' */
} cornetto_step_opt_t;
typedef int (*cornetto_sums_fn)(uint64_t sums[3], void *ctx);
int cornetto_panel_step(cornetto_accel_t *h, const cornetto_asm_t *a, const cornetto_cov_t *c, const cornetto_step_opt_t *opt, cornetto_sums_fn exchange, void *ctx,
                        uint64_t sums[3], int32_t thr[2], cornetto_regpk_t **recs, int64_t *n_recs, int64_t **ctg_first, cornetto_hit_t **hits, int64_t *n_hits,
                        cornetto_win_t **wins, int64_t *n_wins);

/* ---------------------------------------------------------------------------------------------------
 * bedgraph ingest on the device (the text parse of get_depths(), src/boringbits_main.c:204-287)
 * ------------------------------------------------------------------------------------------------- */

typedef struct cornetto_bgin cornetto_bgin_t; /* streaming state of one pair of per-base bedgraphs */

/* which of the reference's checks failed first (smallest record index), with the numbers its message prints */
typedef struct {
    int32_t kind;   /* 1: cov-total record has != 4 columns (a = converted fields)   :209-212
                       2: cov-mq record has != 4 columns (a = converted fields)      :219-222
                       3: "The two files are not in the same order"                  :214-217,:224-227
                       4: not incremental at one base resolution (a = prev_pos, b = start)  :249-252
                       5: end != start + 1 (a = start, b = end)                      :256-259
                       11: a BGZF block of a compressed source (cornetto_bgin_feed_src) is not what its footer says: record = the block's index in
                           its file counted over all feeds, a / b = the low / high 32 bits of blocks[].src as it was handed over, file = the file.
                           Every record that lies wholly in front of the block and has its partner has passed its checks */
    int32_t file;   /* kind 11: 0 cov-total, 1 cov-mq; else 0 (it takes the place of what was padding: no member moved) */
    int64_t record; /* 0-based index of the record */
    int32_t a, b;
} cornetto_bgerr_t;

/* host buffers the device can read at full PCIe rate (for the file pieces handed to cornetto_bgin_feed) */
void *cornetto_pinned_alloc(size_t bytes);
void cornetto_pinned_free(void *p);

int cornetto_bgin_open(cornetto_accel_t *h, cornetto_bgin_t **out);
void cornetto_bgin_close(cornetto_accel_t *h, cornetto_bgin_t *b);

/* Feed the next bytes of cov-total (tot) and cov-mq (mq); any split points, either length may be 0.  Records
 * are four white-space separated tokens exactly as fscanf("%s\t%d\t%d\t%d\n") reads them.  `final` is a bit set:
 * bit 0 = no more cov-total bytes will follow, bit 1 = no more cov-mq bytes.  Like the reference's loop the
 * ingest is done as soon as cov-total is exhausted and every one of its records found its partner
 * (cornetto_bgin_done()).  Returns CORNETTO_OK, or CORNETTO_E_FORMAT when a check of the reference fails
 * (details: cornetto_bgin_error()). */
int cornetto_bgin_feed(cornetto_accel_t *h, cornetto_bgin_t *b, const char *tot, int64_t n_tot, const char *mq, int64_t n_mq,
                       int final);
/* Optional: the pieces the NEXT cornetto_bgin_feed() will be given (pinned memory, untouched until that feed has returned) start their way to the
 * device now, on a copy queue of their own: called in front of a feed, the upload of the next pieces runs beside that feed's kernels (a round of
 * 2 x 64 MB is 4.6 ms of PCIe and ~3 ms of kernels and small read-backs).  The feed that follows with the same pointers and lengths takes the bytes
 * from the device; any other feed waits for the copy and ignores it. */
int cornetto_bgin_prefetch(cornetto_accel_t *h, cornetto_bgin_t *b, const char *tot, int64_t n_tot, const char *mq, int64_t n_mq);
/* bytes of each file handed over but not consumed yet (records without a partner in the other file): a
 * caller that tops both up to the same amount keeps them bounded */
void cornetto_bgin_pending(const cornetto_bgin_t *b, int64_t *pend_tot, int64_t *pend_mq);
/* once the ingest is done: white-space separated tokens of cov-mq behind its last consumed record.  The reference stops reading
 * when cov-total ends (src/boringbits_main.c:204-207) and never sees them; a caller that cuts the files into shares needs the
 * count: leftover tokens in a share that is not the last would have been the partners of the next share's cov-total records. */
int64_t cornetto_bgin_unmatched_mq(const cornetto_bgin_t *b);
const cornetto_bgerr_t *cornetto_bgin_error(const cornetto_bgin_t *b);
int cornetto_bgin_done(const cornetto_bgin_t *b);

/* After a successful final feed: the resident coverage object (ready for cornetto_cov_prepare), the contig
 * names in file order (malloc'd array of malloc'd strings: free() each, then the array) and the number of
 * depth values that were clamped to 65535 (the reference prints a WARNING for each, :261-268). */
int cornetto_bgin_finish(cornetto_accel_t *h, cornetto_bgin_t *b, cornetto_cov_t **cov, int32_t *n_ctg, char ***names,
                         int64_t *n_clamped);

/* ---------------------------------------------------------------------------------------------------
 * run-length bedgraphs on the device: `(no)boringbits --runs`.  An EXTENSION: the reference reads one line per base only
 * (src/boringbits_main.c:256-259 refuses anything else); mosdepth and `bedtools genomecov -bga` write one record per run of equal depth.
 * Defined by expansion: a record `name s e v` stands for the per-base records `name p p+1 v`, p = s .. e-1, and the coverage object is
 * the one cornetto_bgin_finish() gives for the expanded pair.
 * ------------------------------------------------------------------------------------------------- */

typedef struct cornetto_bgrun cornetto_bgrun_t; /* streaming state of one pair of run-length bedgraphs */

/* which check failed: within one file the record with the smallest index decides, within a record the order below */
typedef struct {
    int32_t kind;   /* 1 / 2: a record of cov-total / cov-mq has fewer than 4 converted fields (a = converted fields): header and `track`
                              lines, float values, 1-3 tokens left at the end of the file
                       6: the first run of a contig does not start at 0 (a = start)
                       7: start != previous end within a contig, a gap or an overlap (a = previous end, b = start)
                       8: end <= start (a = start, b = end)
                       9: negative value (a = value)
                       10: at finish, the files disagree: contig `record` is missing in one of them (its length there: 0) or differs in
                           name or length (a, b = its length in cov-total, cov-mq)
                       11: a BGZF block of a compressed source (cornetto_bgrun_feed_src) is not what its footer says: record = the block's index
                           in its file counted over all feeds, a / b = the low / high 32 bits of blocks[].src as it was handed over */
    int32_t file;   /* 0: cov-total, 1: cov-mq */
    int64_t record; /* 0-based index of the record in its file (kind 10: of the contig) */
    int32_t a, b;
} cornetto_bgrunerr_t;

/* positions per workgroup of the expansion kernel (tests plant run and contig seams at its multiples) */
#define CORNETTO_BGRUN_TILE 4096
int32_t cornetto_bgrun_tile(void);

int cornetto_bgrun_open(cornetto_accel_t *h, cornetto_bgrun_t **out);
void cornetto_bgrun_close(cornetto_accel_t *h, cornetto_bgrun_t *b);
/* The next n bytes of file 0 (cov-total) or 1 (cov-mq), ordinary or pinned memory: any split points (inside a token too), the two files in
 * any interleaving; final != 0: the last bytes of that file.  A record is four white-space separated tokens and its numbers convert as in
 * cornetto_bgin_feed().  A record starts a contig iff its name differs from the previous record's in the same file.  Values above 65535
 * are clamped (every position of the run counts as clamped).  CORNETTO_E_FORMAT: cornetto_bgrun_error(). */
int cornetto_bgrun_feed(cornetto_accel_t *h, cornetto_bgrun_t *b, int file, const char *text, int64_t n, int final);
const cornetto_bgrunerr_t *cornetto_bgrun_error(const cornetto_bgrun_t *b);
/* After the final feed of both files: checks them against each other (kind 10), then as cornetto_bgin_finish() — the same kind of
 * object, ready for cornetto_cov_prepare(), the same ownership of the names. */
int cornetto_bgrun_finish(cornetto_accel_t *h, cornetto_bgrun_t *b, cornetto_cov_t **cov, int32_t *n_ctg, char ***names,
                          int64_t *n_clamped);

/* ---------------------------------------------------------------------------------------------------
 * FASTQ reads: record framing of `cornetto seq` / `cornetto sdust reads.fastq` on the device
 * ------------------------------------------------------------------------------------------------- */

/* one plain four-line FASTQ record of the text handed to cornetto_fastq_split(); offsets are into that text */
typedef struct cornetto_fqrec {
    int64_t head;        /* the record's '@'; the name follows it */
    int64_t seq;         /* first base */
    int64_t qual;        /* first quality value */
    int32_t len;         /* bases = quality values (kseq_t.seq.l; a trailing '\r' is dropped as src/kseq.h:138 does) */
    int32_t name_len;    /* kseq_t.name.l: bytes up to the first white space */
    int32_t comment_len; /* kseq_t.comment.l: the comment starts at head + name_len + 2 */
    int32_t keep;        /* 1 if len >= min_len (the test of src/seq.c:120) */
} cornetto_fqrec_t;

/* Frame the FASTQ text `text[0..n)` (host memory, any split point of the file; at most 2^32-256 bytes) the way
 * kseq_read() does (src/kseq.h:184-224 as called by src/seq.c:116 and src/sdust/sdust.c:196) — for as long as the text
 * is made of plain records: '@' line, ONE sequence line, '+' line, ONE quality line of the same length.  That is how
 * basecallers write FASTQ, and for such records the device indexes every line at once instead of walking the bytes.
 *   recs / n_recs   the leading plain records, in input order (cornetto_free)
 *   consumed        bytes of `text` those records cover; hand the rest over again in front of the following bytes
 *   plain           0: what follows at text + consumed is not a plain record (a FASTA record, wrapped sequence or quality,
 *                   blank or stray lines, a quality of another length, the cut-off end of the input) — continue there
 *                   with a sequential kseq reader, which also produces the reference's error behaviour;
 *                   1: only an incomplete record (or nothing) is left, feed more bytes
 *   final           non-zero when no bytes follow `text` (its last line then need not end in a newline)
 *   reads           if not NULL: the bases of the records with len >= min_len, resident in HBM in input order, ready for
 *                   cornetto_sdust_asm() / cornetto_telofind() (cornetto_asm_free) — read i of it is the i-th record
 *                   with keep == 1 */
int cornetto_fastq_split(cornetto_accel_t *h, const char *text, int64_t n, int final, int32_t min_len, cornetto_fqrec_t **recs,
                         int64_t *n_recs, int64_t *consumed, int32_t *plain, cornetto_asm_t **reads);

/* one FASTA record of the text handed to cornetto_fasta_split() */
typedef struct cornetto_farec {
    int64_t head;        /* the record's '>'; the name follows it */
    int64_t len;         /* bases (kseq_t.seq.l): the payload of every line up to the next '>' line */
    int32_t name_len;    /* kseq_t.name.l */
    int32_t pad;
} cornetto_farec_t;

/* The same for FASTA text (kseq_read in front of telofind / sdust / fa2bed: src/find_telomere.c:101, src/sdust/sdust.c:196):
 * `text` must begin with the '>' of a record.  Plain here means that no line begins with '@' or '+' (kseq would read
 * FASTQ there); sequence lines may be wrapped at any width, empty lines and CRLF are handled as kseq does (:138,:202).
 * Unless `final`, the last record of the piece is never returned (it may go on in the following bytes): `consumed` stops
 * at its '>'.  seqs (optional): the sequences of the returned records resident in HBM, newlines removed. */
int cornetto_fasta_split(cornetto_accel_t *h, const char *text, int64_t n, int final, cornetto_farec_t **recs, int64_t *n_recs,
                         int64_t *consumed, int32_t *plain, cornetto_asm_t **seqs);

/* The same over a text that is put on the device slab by slab — a whole uncompressed FASTA file read through a small ring of pinned
 * slabs instead of pinned pieces that must each hold whole records (`cornetto telofind` / `sdust` on an assembly: one framing and one
 * scan for the file; src/find_telomere.c:101, src/sdust/sdust.c:196 read it record by record).  cornetto_text_open(): a device buffer
 * of `capacity` bytes (at most 2^32-256).  cornetto_text_put(): bytes [at, at + n) of the text from `slab` (pinned memory:
 * cornetto_pinned_alloc), asynchronously, on copy queue `slot` (0..3: puts of different slots run side by side — one copy in
 * flight moves ~28 GB/s over PCIe, several ~45); cornetto_text_wait() returns when the last put of that slot has left its slab.  cornetto_fasta_split_text(): waits for every
 * put, then frames the first n bytes exactly as cornetto_fasta_split() frames `text` (head offsets are offsets into the text). */
typedef struct cornetto_text cornetto_text_t;
int cornetto_text_open(cornetto_accel_t *h, int64_t capacity, cornetto_text_t **out);
void cornetto_text_free(cornetto_accel_t *h, cornetto_text_t *t);
int cornetto_text_put(cornetto_accel_t *h, cornetto_text_t *t, const char *slab, int64_t n, int64_t at, int slot);
int cornetto_text_wait(cornetto_accel_t *h, cornetto_text_t *t, int slot);
int cornetto_fasta_split_text(cornetto_accel_t *h, cornetto_text_t *t, int64_t n, int final, cornetto_farec_t **recs, int64_t *n_recs,
                              int64_t *consumed, int32_t *plain, cornetto_asm_t **seqs);

/* ---------------------------------------------------------------------------------------------------
 * BGZF: a bgzip-compressed text inflated on the device (`samtools faidx`-able assembly.fasta.gz in front of telofind / sdust:
 * the reference reads it with gzread() on one thread, src/find_telomere.c:96, src/kseq.h:234)
 * ------------------------------------------------------------------------------------------------- */

/* one BGZF block (a gzip member of at most 64 KiB with its size in the header) */
typedef struct cornetto_bgzf_block {
    int64_t src;   /* offset of its raw deflate stream in the compressed text */
    int64_t dst;   /* offset of its bytes in the inflated text: the sum of n_dst of the blocks before it */
    int32_t n_src; /* bytes of the deflate stream (BSIZE + 1 - header - 8) */
    int32_t n_dst; /* ISIZE of the footer, at most 65536 */
    uint32_t crc;  /* CRC-32 of the footer */
    int32_t pad;
} cornetto_bgzf_block_t;

/* Walk the chain of BGZF members in buf[0 .. n), which are the bytes at offset file_off of the file.  Host only, no device.
 *   dst        in: the inflated offset of the first member; out: that of the member behind the last one returned
 *   blocks     room for `cap` blocks; *n_blocks of them are filled: the members that lie wholly inside the buffer (src counts from the
 *              beginning of the FILE)
 *   resume     file offset of the first member not returned: hand the bytes from there on over next
 *   broken     1: what begins at `resume` is not a BGZF member (another gzip flavour, no `BC` extra subfield, ISIZE above 65536, other
 *              bytes); 0: the buffer or `blocks` ended there */
int cornetto_bgzf_scan(const uint8_t *buf, int64_t n, int64_t file_off, int64_t *dst, cornetto_bgzf_block_t *blocks, int64_t cap,
                       int64_t *n_blocks, int64_t *resume, int32_t *broken);

/* Inflate the blocks from the device text `comp` into the device text `out` (a wave per block: bgzf_inflate) and check every block's
 * CRC-32 (bgzf_crc32).  Waits for the puts of `comp`.  Every block must lie inside its text (CORNETTO_E_ARG otherwise; nothing runs).
 * first_bad: -1, or the lowest index of a block that did not decode to exactly n_dst bytes with the footer's CRC — the status is
 * CORNETTO_E_FORMAT then, the good blocks have their bytes, and a bad block wrote inside its own [dst, dst + n_dst) at most. */
int cornetto_text_inflate(cornetto_accel_t *h, cornetto_text_t *comp, cornetto_text_t *out, const cornetto_bgzf_block_t *blocks,
                          int64_t n_blocks, int64_t *first_bad);

/* The bytes [at[i], at[i] + len[i]) of a device text, i = 0 .. n - 1, packed back to back on the device (one kernel) and copied to dst
 * (one copy; host memory of sum(len) bytes): how the record names of an inflated text reach the host. */
int cornetto_text_gather(cornetto_accel_t *h, cornetto_text_t *t, const int64_t *at, const int32_t *len, int64_t n, char *dst);

/* The other direction: bytes [at, at + n) of the device text `text` as BGZF members in the device text `out` from out_at on, back to back.
 * The bytes are cut every 65280 (0xff00, what bgzip uses; the last member is shorter, n == 0 makes no member) and a wave makes a member
 * (bgzf_deflate): one dynamic-Huffman block whose only matches are byte runs (a run of one value of 4 or more bytes is its first byte and
 * distance-1 matches), or one stored block where that would not be smaller, so a member has at most 65280 + 5 + 26 = 65311 bytes; header
 * with `BC`/BSIZE, CRC-32 and ISIZE as bgzip writes them.  The members' sizes are scanned (bgzf_scan) and the members packed (bgzf_pack).
 * No end-of-file block is written.  `out` must have room for ceil(n / 65280) * 65536 bytes behind out_at: CORNETTO_E_ARG otherwise, and
 * nothing runs.  Waits for the puts of `text`.  *n_out: bytes of the chain, *n_members: its members.  The bytes depend on the text alone. */
int cornetto_text_deflate(cornetto_accel_t *h, cornetto_text_t *text, int64_t at, int64_t n, cornetto_text_t *out, int64_t out_at, int64_t *n_out,
                          int64_t *n_members);

/* Bedgraph text from a bgzip-compressed depth file (mosdepth writes *.per-base.bed.gz only): the next bytes of one file for the two bedgraph
 * readers, either plain bytes in host memory or the next BGZF blocks of the file, whose deflate streams are on the device.  The feed gives a
 * compressed source's blocks their places behind the bytes it carries over from the last feed IN THE READER'S OWN TEXT WORKSPACE, inflates
 * them there (bgzf_inflate, bgzf_crc32) and tokenises in place: inflated text never crosses PCIe, and from the first compressed source of a
 * file on, what is carried over between its feeds stays on the device.  n == 0 && n_blocks == 0 (or a NULL source): nothing new for the
 * file.  A source with both is CORNETTO_E_ARG, and so is a block that lies outside `comp` or says more than 65536 bytes. */
typedef struct cornetto_bgsrc {
    const char *text; int64_t n;                 /* plain bytes in host memory (ordinary or pinned), or */
    cornetto_text_t *comp;                       /* a device text holding deflate streams, put there with cornetto_text_put() */
    const cornetto_bgzf_block_t *blocks;         /* the next blocks of the file in file order: src = offsets into comp, dst ignored */
    int64_t n_blocks;
} cornetto_bgsrc_t;
/* cornetto_bgin_feed() / cornetto_bgrun_feed() over such sources: the same records, checks, results and errors; the two files of a pair may be
 * of different kinds, and a file may change kind between feeds.  The limit of 0xF0000000 bytes per file and feed counts carried plus inflated
 * bytes (the sum of n_dst): CORNETTO_E_ARG beyond, before anything runs.  Synchronous: `comp` may be overwritten on return.
 * A damaged block is kind 11 of cornetto_bgerr_t / cornetto_bgrunerr_t: what is reported is that block or a failed check of a record that lies
 * wholly in front of it, never anything made from its bytes or from bytes behind it, and no depth value from such bytes is stored. */
int cornetto_bgin_feed_src(cornetto_accel_t *h, cornetto_bgin_t *b, const cornetto_bgsrc_t *tot, const cornetto_bgsrc_t *mq, int final);
int cornetto_bgrun_feed_src(cornetto_accel_t *h, cornetto_bgrun_t *b, int file, const cornetto_bgsrc_t *src, int final);

/* ---------------------------------------------------------------------------------------------------
 * BAM: both per-base coverage tracks from a coordinate-sorted or unsorted BAM on the device: `(no)boringbits --bam`.  An EXTENSION (the
 * reference's `depth` sub-command is a stub; the protocol runs `samtools depth -aa` and `samtools depth -Q 20 -aa` through awk).  The rules,
 * a restatement of those two commands:
 *   - contigs, their order and lengths: the binary reference list of the header; every contig appears, with or without reads;
 *   - a record counts iff refID >= 0 and (flag & skip_flags) == 0 (0x704: UNMAP, SECONDARY, QCFAIL, DUP); it counts in the second track iff
 *     also mapq >= min_mapq;
 *   - its CIGAR is walked from pos: M = X count and advance, D N advance, I S H P (and the op codes 9-15) do neither; positions are cut to
 *     [0, contig length); n_cigar_op == 0 covers nothing;
 *   - n_cigar_op == 2 with the ops `<l_seq>S <x>N`: the CIGAR is the CG:B,I array of the auxiliary fields if there is one;
 *   - depth above 65535 is stored as 65535 and counted (n_clamped).  No base-quality filter, no overlap handling.
 * ------------------------------------------------------------------------------------------------- */

/* The header of a BAM in buf[0 .. n), the first inflated bytes of the file.  Host only.  CORNETTO_OK: *n_ref contigs with names[i]
 * (malloc: free every name, then the array) and lens[i] (malloc), *header_bytes = where the first record begins.  1: the header goes on
 * behind buf, hand over more bytes (nothing is allocated).  CORNETTO_E_FORMAT: not a BAM header (magic, a negative count or length). */
int cornetto_bam_header(const uint8_t *buf, int64_t n, int32_t *n_ref, char ***names, int32_t **lens, int64_t *header_bytes);

typedef struct {
    int32_t min_mapq;    /* second track: mapq >= this (20) */
    uint32_t skip_flags; /* a record with one of these flag bits does not count (0x704) */
    int64_t window;      /* bytes of inflated BAM held on the device at once: an operating parameter, never changes a result.  It must hold
                            the largest record and one BGZF block more (CORNETTO_E_NOMEM otherwise) */
    int32_t records;     /* 0: depth only; 1: also keep the record table (cornetto_bam_records); 2: the record table only — no depth array is
                            allocated and cornetto_bamdepth_finish() returns no coverage object */
    int32_t pad;
} cornetto_bamdepth_opt_t;
void cornetto_bamdepth_defaults(cornetto_bamdepth_opt_t *opt);

/* which check failed; the record with the smallest index decides, within a record the order below */
typedef struct {
    int32_t kind;   /* 1: block_size < 32 (a = block_size)
                       2: the file ends inside a record (a = bytes left, b = the record's block_size, -1 if that is cut off too); the callers
                          of cornetto_bam_header() report a file that ends inside its header as kind 2 of record -1, and bytes that are no BAM
                          header as kind 7
                       3: the fixed fields say more than block_size: 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq (a, capped at
                          2^31-1) > block_size (b)
                       4: refID (a) outside [-1, n_ref (b))
                       5: the CG:B,I array of a long-CIGAR record has more elements (a, capped) than the record has room for (b, bytes)
                       6: BGZF block a of the file (counted from 0 over all feeds) is not what its footer says; every record that lies
                          wholly in front of it has passed its checks; record = the number of those records */
    int32_t a, b;
    int32_t pad;
    int64_t record; /* 0-based index of the record in the file */
} cornetto_bamerr_t;

/* one record as the depth kernel read it */
typedef struct {
    int64_t offset;  /* of its block_size field in the inflated file */
    int32_t ref_id, pos, mapq, flag;
    int32_t counted; /* 1 if it counts in the first track */
    int32_t n_ops;   /* CIGAR operations walked (those of the CG array for a long-CIGAR record); 0 for a record that does not count */
    int64_t span;    /* reference bases its CIGAR advances over (0 for a record that does not count: its CIGAR is not walked) */
    int64_t bases;   /* positions it adds one to: its M = X bases inside [0, contig length) */
} cornetto_bamrec_t;

/* positions per workgroup of the scan kernel (tests plant contig and read ends at its multiples) */
#define CORNETTO_BAM_SCAN_TILE 4096
int32_t cornetto_bam_scan_tile(void);

typedef struct cornetto_bamdepth cornetto_bamdepth_t;
/* lens[0 .. n_ref): the contig lengths of the header.  Allocates two int32 difference arrays over all contigs (records != 2). */
int cornetto_bamdepth_open(cornetto_accel_t *h, const cornetto_bamdepth_opt_t *opt, const int32_t *lens, int32_t n_ref, cornetto_bamdepth_t **out);
void cornetto_bamdepth_close(cornetto_accel_t *h, cornetto_bamdepth_t *b);
/* The next BGZF blocks of the file, in file order: `comp` holds their deflate streams at blocks[i].src (offsets into `comp`; dst is
 * ignored: the blocks follow each other), put there with cornetto_text_put().  skip: inflated bytes to pass over before the first record
 * (the header: cornetto_bam_header()), counted from the first block of the file: only a feed in front of the first record may skip
 * (CORNETTO_E_ARG afterwards).  Blocks are inflated a window at a time
 * (cornetto_text_inflate), records framed (bam_frame) and their CIGARs walked into the difference arrays (bam_depth); the bytes behind the
 * last whole record of a window stay in front of the next one, across feeds too.  Synchronous: `comp` may be overwritten on return. */
int cornetto_bamdepth_feed(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_text_t *comp, const cornetto_bgzf_block_t *blocks, int64_t n_blocks,
                           int64_t skip);
const cornetto_bamerr_t *cornetto_bamdepth_error(const cornetto_bamdepth_t *b);
/* After the last feed (a file that ends inside a record: kind 2): the difference arrays are scanned and clamped (bam_scan) into the
 * coverage object cornetto_cov_wrap() makes, ready for cornetto_cov_prepare().  n_records: records of the file; n_counted: those that count
 * in the first track; n_clamped: positions above 65535 in either track.  Any of the three may be NULL. */
int cornetto_bamdepth_finish(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_cov_t **cov, int64_t *n_records, int64_t *n_counted,
                             int64_t *n_clamped);
/* The record table of the feeds so far (opt.records != 0), in file order: cornetto_free(). */
int cornetto_bam_records(cornetto_accel_t *h, cornetto_bamdepth_t *b, cornetto_bamrec_t **recs, int64_t *n_recs);

/* ---------------------------------------------------------------------------------------------------
 * BAM to FASTQ: the length-filtered FASTQ text of a basecaller's (unaligned or aligned) BAM on the device: `seq --bam`.  An EXTENSION (the
 * reference's `seq` reads FASTQ text, src/seq.c:63-129; the protocol leaves the step from dorado's BAM to that text to the user, who runs
 * `samtools view -d dx:1 | samtools fastq` in front of it).  The rules:
 *   - records are taken in file order; the header is skipped with cornetto_bam_header() (no reference contig is the normal case); the checks
 *     of cornetto_bamerr_t kinds 1, 2, 3, 4 and 6 apply unchanged, and nothing of a record is printed before its checks have passed;
 *   - a record with flag & 0x900 (SECONDARY, SUPPLEMENTARY) is passed over: it counts nowhere.  Every other record counts in `total reads`
 *     with l_seq bases;
 *   - a record is kept iff l_seq >= min_len and, with `duplex`, it has an auxiliary field dx of an integer type (c C s S i I) with the value
 *     1.  The search obeys the rule of the CG search: every field is checked against the record's end before it is read, fields that do not
 *     parse end the search; a dx of any other type is no tag;
 *   - a kept record prints as "@name\nBASES\n+\nQUALITIES\n" (what src/seq.c:120-129 prints for a record without a comment):
 *     name: the first l_read_name - 1 bytes of read_name (none if l_read_name is 0); bases: "=ACMGRSVTWYHKDBN"[nibble], high nibble first;
 *     qualities: min(q, 93) + 33, and if the first quality byte is 0xFF they are absent and every one prints as '"' (samtools fastq -v 1);
 *   - flag & 0x10 reverses the bases and complements them with "=TGKCYSBAWRDMHVN", and reverses the qualities;
 *   - so l_seq == 0 with min_len 0 prints "@name\n\n+\n\n".
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t min_len;     /* keep l_seq >= this (30000: src/seq.c:63) */
    int32_t duplex;      /* non-zero: keep only records with dx:1 */
    int64_t window;      /* bytes of inflated BAM held on the device at once, at most 2^31: an operating parameter, never changes a result.
                            It must hold the largest record and one BGZF block more (CORNETTO_E_NOMEM otherwise) */
    int32_t n_ref;       /* reference contigs of the header (check 4) */
    int32_t records;     /* non-zero: keep the record table (cornetto_bamfq_records) */
} cornetto_bamfq_opt_t;
void cornetto_bamfq_defaults(cornetto_bamfq_opt_t *opt);

/* one record as the size pass read it */
typedef struct {
    int64_t offset;   /* of its block_size field in the inflated file */
    int32_t l_seq, flag, name_len;
    int32_t kept;     /* 1: printed; 0: too short or without dx:1; -1: passed over (flag & 0x900) */
} cornetto_bamfqrec_t;

typedef struct cornetto_bamfq cornetto_bamfq_t;
int cornetto_bamfq_open(cornetto_accel_t *h, const cornetto_bamfq_opt_t *opt, cornetto_bamfq_t **out);
void cornetto_bamfq_close(cornetto_accel_t *h, cornetto_bamfq_t *b);
/* ONE window: the leading blocks of blocks[0 .. n_blocks) that fit behind the tail the last window left (*taken of them; blocks, comp and
 * skip as in cornetto_bamdepth_feed()) are inflated and framed, every record checked and sized (bamfq_size: name_len + 2 l_seq + 6 bytes
 * for a kept record, 0 otherwise), the sizes scanned into text offsets (scan.hpp).  *n_text: bytes of the window's text, ready for
 * cornetto_bamfq_get() until the next feed.  CORNETTO_E_FORMAT (cornetto_bamfq_error(); the record with the lowest index decides): the
 * window's text is that of the records in front of the failing one, and may be fetched; no further feed is taken.  CORNETTO_E_NOMEM with
 * *taken == 0: the first block does not fit the window behind the carried bytes.  Synchronous: `comp` may be overwritten on return. */
int cornetto_bamfq_feed(cornetto_accel_t *h, cornetto_bamfq_t *b, cornetto_text_t *comp, const cornetto_bgzf_block_t *blocks, int64_t n_blocks,
                        int64_t skip, int64_t *taken, int64_t *n_text);
/* Bytes [at, at + n) of the window's text into `dst_pinned` (cornetto_pinned_alloc), through a device slab (bamfq_text: a workgroup writes a
 * tile of the text, a thread 16 bytes) on copy slot 0..3, asynchronously as cornetto_emit_get(): the copy of one slab runs beside the
 * kernel of the next.  cornetto_bamfq_wait(): the last get of the slot is in its buffer.  Every get of a window ends before the next feed
 * (the feed waits for all four slots). */
int cornetto_bamfq_get(cornetto_accel_t *h, cornetto_bamfq_t *b, char *dst_pinned, int64_t at, int64_t n, int slot);
int cornetto_bamfq_wait(cornetto_accel_t *h, cornetto_bamfq_t *b, int slot);
/* The same range of the window's text as BGZF members (`seq --bam --bgzf`): the slab bamfq_text writes is deflated on the device under the
 * rules of cornetto_text_deflate() and only the packed members reach `dst_pinned`, which must have dst_cap >= ceil(n / 65280) * 65536 bytes
 * (CORNETTO_E_ARG otherwise, nothing runs).  The same four slots; a slot carries one get of either kind at a time.
 * cornetto_bamfq_wait_bgzf(): the members of the slot's last such get are in its buffer, *n_bytes of them (0 after a get of no bytes). */
int cornetto_bamfq_get_bgzf(cornetto_accel_t *h, cornetto_bamfq_t *b, char *dst_pinned, int64_t dst_cap, int64_t at, int64_t n, int slot);
int cornetto_bamfq_wait_bgzf(cornetto_accel_t *h, cornetto_bamfq_t *b, int slot, int64_t *n_bytes);
/* After the last feed: a file that ends inside a record is kind 2. */
int cornetto_bamfq_finish(cornetto_accel_t *h, cornetto_bamfq_t *b);
/* stats[0 .. 5): reads and bases of `total reads`, reads and bases of `reads >= min_len`, then the records taken (the passed-over ones
 * among them), over the feeds so far (on an error: of the records in front of the failing one) */
void cornetto_bamfq_stats(const cornetto_bamfq_t *b, int64_t *stats);
const cornetto_bamerr_t *cornetto_bamfq_error(const cornetto_bamfq_t *b);
/* The record table of the feeds so far (opt.records), in file order: cornetto_free(). */
int cornetto_bamfq_records(cornetto_accel_t *h, cornetto_bamfq_t *b, cornetto_bamfqrec_t **recs, int64_t *n_recs);

/* ---------------------------------------------------------------------------------------------------
 * FASTQ to FASTQ: the length-filtered text `cornetto seq -m` prints (src/seq.c:116-129), written on the device from FASTQ text that is plain
 * bytes or BGZF blocks: `seq --fastq`.  The object, its window, its four copy slots and its two kinds of get are those of cornetto_bamfq_*;
 * the records and what makes one plain are those of cornetto_fastq_split() (the same kernel).  A kept record (len >= min_len) prints as
 *   '@' name [TAB comment] '\n' bases "\n+\n" qualities '\n'
 * the TAB in place of whatever white-space byte stood between name and comment, none when the comment is empty; a trailing '\r' of the three
 * payload lines, whatever follows '+' on the third line and the separator itself are not copied.  A record that holds a byte 0 is not plain
 * for this stage (the reference prints with "%s"): it and everything behind it are the caller's sequential reader's.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t min_len;     /* keep len >= this (30000: src/seq.c:63) */
    int32_t records;     /* non-zero: keep the record table (cornetto_fqseq_records) */
    int64_t window;      /* bytes of FASTQ text held on the device at once, at most 2^32-256 (the newline table is uint32), 256 MiB by default: an
                            operating parameter, never changes a result.  It must hold the largest record, and for BGZF blocks one block more */
} cornetto_fqseq_opt_t;
void cornetto_fqseq_defaults(cornetto_fqseq_opt_t *opt);

/* output bytes per workgroup of the text kernel (tests plant every part of a record at its multiples) */
#define CORNETTO_FQSEQ_TILE 16384
int32_t cornetto_fqseq_tile(void);

typedef struct cornetto_fqseq cornetto_fqseq_t;
int cornetto_fqseq_open(cornetto_accel_t *h, const cornetto_fqseq_opt_t *opt, cornetto_fqseq_t **out);
void cornetto_fqseq_close(cornetto_accel_t *h, cornetto_fqseq_t *q);
/* ONE window.  src: the next bytes of the stream, plain or BGZF blocks, under the contract of cornetto_bgin_feed_src() (NULL or empty: nothing
 * new).  *taken: the leading bytes (plain) or blocks (BGZF) that fit the window behind the tail the last window left; hand the others over
 * again.  final: nothing follows `src` (it counts once all of src is taken: the last line then need not end in a newline).  The text is
 * indexed, framed, sized and scanned; *n_text: bytes of the window's text, ready for cornetto_fqseq_get() until the next feed.  What follows
 * the last whole record stays on the device in front of the next window.  *plain = 0: the first group of four lines that is not a plain
 * record (or, with `final`, whatever follows the last one) ends the device's part: the window's text and the counts cover the records in
 * front of it, cornetto_fqseq_rest() says where the sequential reader continues, and no further feed is taken (CORNETTO_E_ARG).
 * CORNETTO_E_FORMAT: a damaged BGZF block (cornetto_fqseq_error(): its index in the file, counted over all feeds); the window's text is that of
 * the records that lie wholly in front of the block and may be fetched; no further feed is taken.  CORNETTO_E_NOMEM with *taken == 0: not one
 * more byte (or block) fits behind the carried bytes: a record larger than the window.  Synchronous: `src` may be overwritten on return. */
int cornetto_fqseq_feed(cornetto_accel_t *h, cornetto_fqseq_t *q, const cornetto_bgsrc_t *src, int final, int64_t *taken, int64_t *n_text, int32_t *plain);
/* offset in the plain or inflated stream of the first byte that no record of the feeds so far holds */
int64_t cornetto_fqseq_rest(const cornetto_fqseq_t *q);
/* -1, or the index of the damaged block */
int64_t cornetto_fqseq_error(const cornetto_fqseq_t *q);
/* The two kinds of get, with the contracts (slots, dst_cap, waits) of cornetto_bamfq_get() / _wait() and cornetto_bamfq_get_bgzf() / _wait_bgzf():
 * fqseq_text writes the slab, a workgroup a tile of CORNETTO_FQSEQ_TILE bytes, a thread 16 bytes. */
int cornetto_fqseq_get(cornetto_accel_t *h, cornetto_fqseq_t *q, char *dst_pinned, int64_t at, int64_t n, int slot);
int cornetto_fqseq_wait(cornetto_accel_t *h, cornetto_fqseq_t *q, int slot);
int cornetto_fqseq_get_bgzf(cornetto_accel_t *h, cornetto_fqseq_t *q, char *dst_pinned, int64_t dst_cap, int64_t at, int64_t n, int slot);
int cornetto_fqseq_wait_bgzf(cornetto_accel_t *h, cornetto_fqseq_t *q, int slot, int64_t *n_bytes);
/* stats[0 .. 5): reads and bases of `total reads`, reads and bases of `reads >= min_len`, then the records taken, over the feeds so far */
void cornetto_fqseq_stats(const cornetto_fqseq_t *q, int64_t *stats);
/* The record table of the feeds so far (opt.records), in input order, offsets into the stream: cornetto_free(). */
int cornetto_fqseq_records(cornetto_accel_t *h, cornetto_fqseq_t *q, cornetto_fqrec_t **recs, int64_t *n_recs);
/* Waits for every get; *ms: the time of the fqseq_text launches so far that ran under cornetto_accel_set_timing(2), *n_bytes: what they wrote. */
int cornetto_fqseq_text_time(cornetto_accel_t *h, cornetto_fqseq_t *q, double *ms, int64_t *n_bytes);

/* ---------------------------------------------------------------------------------------------------
 * The mean-quality filter of `seq -q` (not in the reference), for cornetto_fqseq_* and cornetto_bamfq_* and every host loop.  THE RULE:
 *   - weights: E[q] = round(10^9 * 10^(-q/10)) for q = 0 .. 93, the literal table below (no entry is a rounding tie: 10^(-q/10) is irrational
 *     unless q is a multiple of 10, and then the value is an integer);
 *   - a character c of a printed FASTQ quality line has q = clamp(c - 33, 0, 93): bytes below '!' give 0, bytes above '~' give 93;
 *   - with S = the sum of E[q] over the PRINTED quality characters and L = the number of printed bases, a read passes iff S <= P * L.
 *     P, an integer in [0, 10^9], is the largest mean error probability allowed in units of 10^-9; L < 2^31, so both sides fit 64 bits.
 *     64-bit integers only, no floating point on any path; the sum does not depend on the order, so device, host and tests agree bit for bit;
 *   - a read is printed iff it passes the length filter, and --duplex where given, and this.  L = 0 passes; a record printed with an empty
 *     quality line (a FASTA record through `seq FILE`) passes;
 *   - BAM: the characters are the ones `seq --bam` prints: q = min(raw, 93); absent qualities (first byte 0xFF) print as '"' each, so
 *     S = l_seq * E[1]; reversing the qualities does not change the sum.  `seq --bam F -q T` prints what
 *     `seq --bam F -m .. | seq --fastq - -m 0 -q T` prints.
 * NOT replicated: dorado's --min-qscore skips the first 60 bases and has its qs tag; neither is copied.  Parity with dorado, chopper or
 * samtools is unpinned, like every other extension here.
 * On the device (qmean_sum, csrc/qmean.hpp): a wave owns 1 KiB of the window, finds the quality ranges that reach into it and adds every
 * range's weights to its 64-bit sum; a pass per record then clears the keep decision where S > P * L, in front of the size scan.
 * ------------------------------------------------------------------------------------------------- */
#define CORNETTO_QUAL_MAX 93
#define CORNETTO_QUAL_ONE 1000000000ll /* E[0]: the unit of P */
#define CORNETTO_QUAL_WEIGHTS                                                                                   \
    {                                                                                                           \
        1000000000u, 794328235u, 630957344u, 501187234u, 398107171u, 316227766u, 251188643u, 199526231u,        \
        158489319u, 125892541u, 100000000u, 79432823u, 63095734u, 50118723u, 39810717u, 31622777u,              \
        25118864u, 19952623u, 15848932u, 12589254u, 10000000u, 7943282u, 6309573u, 5011872u,                    \
        3981072u, 3162278u, 2511886u, 1995262u, 1584893u, 1258925u, 1000000u, 794328u,                          \
        630957u, 501187u, 398107u, 316228u, 251189u, 199526u, 158489u, 125893u,                                 \
        100000u, 79433u, 63096u, 50119u, 39811u, 31623u, 25119u, 19953u,                                        \
        15849u, 12589u, 10000u, 7943u, 6310u, 5012u, 3981u, 3162u,                                              \
        2512u, 1995u, 1585u, 1259u, 1000u, 794u, 631u, 501u,                                                    \
        398u, 316u, 251u, 200u, 158u, 126u, 100u, 79u,                                                          \
        63u, 50u, 40u, 32u, 25u, 20u, 16u, 13u,                                                                 \
        10u, 8u, 6u, 5u, 4u, 3u, 3u, 2u,                                                                        \
        2u, 1u, 1u, 1u, 1u, 1u                                                                                  \
    }
/* E[clamp(q, 0, 93)] */
uint32_t cornetto_qual_weight(int q);
/* Between open and the first feed: P = -1 turns the filter off (the default: nothing of it is launched or allocated), 0 .. 10^9 sets it.
 * CORNETTO_E_ARG after a feed or out of range. */
int cornetto_fqseq_set_max_err(cornetto_accel_t *h, cornetto_fqseq_t *q, int64_t P);
int cornetto_bamfq_set_max_err(cornetto_accel_t *h, cornetto_bamfq_t *b, int64_t P);
/* qstats[0 .. 2): reads and bases printed, over the feeds so far (with the filter off: those of `reads >= min_len`).  With the filter on
 * the `keep` / `kept` column of the record tables is 1 exactly for the printed records; the counts of cornetto_*_stats() keep their
 * meaning (length, and dx for a BAM). */
void cornetto_fqseq_qstats(const cornetto_fqseq_t *q, int64_t *qstats);
void cornetto_bamfq_qstats(const cornetto_bamfq_t *b, int64_t *qstats);
/* The sums S of the feeds so far, a uint64_t per record in the order of the record table (opt.records and the filter on; CORNETTO_E_ARG
 * otherwise); a record dropped before the sum (length, dx, passed over) reports 0: cornetto_free(). */
int cornetto_fqseq_qsums(cornetto_accel_t *h, cornetto_fqseq_t *q, uint64_t **sums, int64_t *n_sums);
int cornetto_bamfq_qsums(cornetto_accel_t *h, cornetto_bamfq_t *b, uint64_t **sums, int64_t *n_sums);

/* ---------------------------------------------------------------------------------------------------
 * k-mer QV of an assembly against a truth set: `cornetto qv`.  An EXTENSION (the reference's protocol runs `yak count` / `yak qv` against the
 * HG002 Q100 assembly at this step, docs/protocol.md:292-303; yak's histogram error model is NOT replicated, the rule below is Merqury's;
 * parity with either is unpinned).  THE RULE:
 *   - k is odd, 11 <= k <= 31 (default 21): no k-mer is its own reverse complement;
 *   - base codes: A a = 0, C c = 1, G g = 2, T t = 3; every other byte is invalid;
 *   - position i of a contig of length L holds a k-mer iff i + k <= L and all of seq[i .. i + k) are valid;
 *   - the k-mer is canonical: min(fwd, rc) of the two 2k-bit codes, first base most significant;
 *   - the truth set S: the canonical k-mers of every position of every record of the truth file(s);
 *   - per contig c of an assembly: kmers[c] = the positions that hold a k-mer, counted with multiplicity; missing[c] = those of them whose
 *     canonical k-mer is not in S;
 *   - per contig, on request: the union of the spans [i, i + k) of the missing positions; spans that overlap or are book-ended merge
 *     (bedtools merge); rows cornetto_ivl_t {ctg, start, finish} by contig, then by start;
 *   - QV, on the host in double from the two integers: p = (kmers - missing) / kmers, e = 1 - pow(p, 1.0 / k), qv = -10 log10(e); missing == 0
 *     prints e as 0 and qv as inf, kmers == 0 prints both as NA, otherwise e with %.3e and qv with %.2f.
 * Every count is an integer that does not depend on the order of insertion or of the probes.
 * On the device (csrc/kqv.hip, kqv.hpp): an open-addressing table of uint64_t with linear probing, the empty slot ~0, the home slot
 * mulhi64(mix(key), slots) — slots need not be a power of two; a contig is cut into tiles of CORNETTO_KQV_TILE bases, a workgroup a tile.
 * ------------------------------------------------------------------------------------------------- */
#define CORNETTO_KQV_TILE 4096
typedef struct cornetto_kset cornetto_kset_t; /* a set of canonical k-mers resident in HBM */
/* slots >= 1 (8 bytes each); a k outside the rule: CORNETTO_E_UNSUPPORTED; a table that cannot be allocated: CORNETTO_E_NOMEM, the message says
 * how many bytes were wanted.  Every slot is set to empty on the handle's stream, whatever the memory held. */
int cornetto_kset_open(cornetto_accel_t *h, int32_t k, int64_t slots, cornetto_kset_t **out);
/* the k-mers of every contig of `truth` into the set (kq_insert); may be called repeatedly, once per batch of a streamer.  CORNETTO_E_NOMEM: the
 * table overflowed (a probe found no room in `slots` steps), the set is unusable from then on.  Never a hang: no probe takes more steps. */
int cornetto_kset_add(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *truth);
/* stats[0 .. 3): positions inserted (with multiplicity), distinct k-mers, slots */
void cornetto_kset_stats(const cornetto_kset_t *s, int64_t *stats);
/* kmers[c], missing[c] for the contigs of `a` (kq_query; arrays of the assembly's contig count).  runs / n_runs (both or neither): the rows of
 * the rule, cornetto_free().  The rows are placed by 32-bit counts: with rows requested, an assembly with bases / 2 + contigs > 2^32 - 1 is
 * refused by its size alone (CORNETTO_E_UNSUPPORTED).  One call at a time per set: the set keeps the call's tile table. */
int cornetto_kset_query(cornetto_accel_t *h, const cornetto_kset_t *s, const cornetto_asm_t *a, int64_t *kmers, int64_t *missing, cornetto_ivl_t **runs,
                        int64_t *n_runs);
void cornetto_kset_free(cornetto_accel_t *h, cornetto_kset_t *s);

/* ---------------------------------------------------------------------------------------------------
 * Counted k-mer sets: the truth of `cornetto qv -r` and `cornetto trioeval --pat-reads / --mat-reads` from READS, whose k-mers are evidence only
 * from a count threshold upward (Merqury works this way; the reference's protocol builds `yak` indexes of parental reads, docs/protocol.md:292-308;
 * parity with either is unpinned).  Extraction is the rule of `cornetto qv` above, unchanged: the same valid bytes, canonical code and positions.
 * THE RULE:
 *   - a counted set has `channels` = 1 or 2.  Channel 0 is the truth of `qv`; for `trioeval`, channel 0 is pat and channel 1 is mat;
 *   - count[ch][key] = min(occurrences of key at the positions of every record counted into channel ch, CORNETTO_KSET_COUNT_CAP): an integer that
 *     does not depend on batch boundaries, on the order of the records or on the order of the probes;
 *   - hist[ch][c], c = 1 .. CORNETTO_KSET_HIST_BINS - 1: the number of distinct keys with min(count[ch][key], BINS - 1) == c.  Bin 0 is unused and
 *     stays 0; the last bin collects every count from BINS - 1 up;
 *   - sealing with thresholds m[ch] >= 1: key x is SOLID in ch iff count[ch][x] >= m[ch]; S_ch = the solid keys of channel ch, solid[ch] = |S_ch|.
 *     With one channel the set becomes the plain set S_0, and cornetto_kset_query() answers exactly as a plain set filled with S_0 would.  With two
 *     it becomes the tagged set with tag = (x in S_0 ? PAT : 0) | (x in S_1 ? MAT : 0); keys with tag 0 are absent, and cornetto_kset_phase()
 *     answers as a tagged set built from S_0 and S_1 would;
 *   - hence with m = 1 and every record counted once, the result is that of cornetto_kset_add() / cornetto_kset_add_tag() on the same records.
 * The state machine; a call out of order returns CORNETTO_E_UNSUPPORTED, a null object CORNETTO_E_ARG: kset_count and kset_hist only before the
 * seal, kset_query (one channel) and kset_phase (two) only after it, kset_add and kset_add_tag never on a counted set, kset_seal once.  A set whose
 * table has overflowed refuses everything, as a plain one does.
 * On the device (csrc/kcount.hip, kqv.hpp): the table of `qv` with channels * slots uint32_t counts beside it (12 or 16 bytes per slot), added
 * with one atomic per k-mer; lanes are dealt runs of the batch's records, not records, so 150-base reads fill the waves; sealing rewrites the
 * table in place and frees the counts, a key that is solid nowhere leaves a tombstone that no key equals and every walk passes.
 * ------------------------------------------------------------------------------------------------- */
#define CORNETTO_KSET_COUNT_CAP 65535
#define CORNETTO_KSET_HIST_BINS 1024
/* cornetto_kset_open() for a counted set of `channels` (1 or 2, else CORNETTO_E_ARG) channels: the table emptied and the counts zeroed on the
 * handle's stream, whatever the memory held.  CORNETTO_E_NOMEM: the message says how many bytes were wanted (8 + 4 * channels per slot). */
int cornetto_kset_open_counted(cornetto_accel_t *h, int32_t k, int64_t slots, int32_t channels, cornetto_kset_t **out);
/* the k-mers of every record of `reads` counted into `channel` (kq_count); may be called repeatedly, once per batch of a streamer.  Overflow as
 * in cornetto_kset_add(): CORNETTO_E_NOMEM, the set is unusable, never a hang.  cornetto_kset_stats(): positions counted (all channels), distinct
 * keys counted, slots. */
int cornetto_kset_count(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *reads, int32_t channel);
/* hist[0 .. CORNETTO_KSET_HIST_BINS) of `channel` (kq_hist) */
int cornetto_kset_hist(cornetto_accel_t *h, cornetto_kset_t *s, int32_t channel, int64_t *hist);
/* min_count[0 .. channels), each 1 .. CORNETTO_KSET_COUNT_CAP (else CORNETTO_E_ARG); solid[0 .. channels) (kq_seal).  The counts are freed. */
int cornetto_kset_seal(cornetto_accel_t *h, cornetto_kset_t *s, const int32_t *min_count, int64_t *solid);

/* ---------------------------------------------------------------------------------------------------
 * k-mer completeness and copy-number spectrum of an assembly against the counted reads: `cornetto qv -r ... --completeness --spectra-cn FILE`.
 * An EXTENSION (Merqury's completeness and spectra-cn classes; parity with Merqury or yak is unpinned).  k, the valid bytes, the positions and
 * the canonical code are those of `cornetto qv` above.  A counted set of ONE channel, BEFORE its seal, may additionally hold copies[key].
 * THE RULE:
 *   - copies[key] = min(occurrences of key at the positions of every contig handed to cornetto_kset_copies() since the last clear,
 *     CORNETTO_KSET_CN_BINS - 1).  The classes are Merqury's: read-only (0), 1, 2, 3, 4, more than 4;
 *   - a key of the assembly that the table does not hold is inserted with count 0: an ASSEMBLY-ONLY key.  It takes a slot; a table without room is
 *     the overflow status of cornetto_kset_count() (CORNETTO_E_NOMEM, the set unusable, never a hang);
 *   - assembly-only keys do not count in the distinct keys of cornetto_kset_stats(), they are in no bin of cornetto_kset_hist() (which skips count 0),
 *     and the seal turns them into tombstones: a set that has seen copies calls seals into exactly the set it would have sealed into without
 *     them, and every later cornetto_kset_query() answer is the same;
 *   - spec[a * CORNETTO_KSET_HIST_BINS + c], a = 0 .. CORNETTO_KSET_CN_BINS - 1, c = 0 .. CORNETTO_KSET_HIST_BINS - 1: the number of keys with
 *     min(copies, CN_BINS - 1) == a and min(count, HIST_BINS - 1) == c.  The cell a = 0, c = 0 stays 0 (a key that is in neither, e.g. an
 *     assembly-only key of an earlier assembly after a clear); row c = 0 is the assembly-only keys; for c >= 1 the sum over a of spec[a][c] is
 *     hist[c]; before any copies call spec[0][c] == hist[c];
 *   - with a threshold m in 1 .. CORNETTO_KSET_COUNT_CAP: solid = the keys with min(count, CAP) >= m, which is what the seal with m will return;
 *     found = those of them with copies >= 1.  Both are exact for every m, also above HIST_BINS - 1 where the bins no longer tell;
 *   - completeness = found / solid, on the host in double, printed with %.6f, or NA when solid is 0.
 * Every number is an integer independent of batch boundaries and of the order of records, contigs and probes.
 * The state machine: kset_copies, kset_copies_clear and kset_spectrum on a plain, tagged, sealed or two-channel set return
 * CORNETTO_E_UNSUPPORTED; so does kset_count after the first kset_copies (the distinct-keys stat would no longer mean what it says); a channel
 * out of range, m outside 1 .. CAP and null arguments are CORNETTO_E_ARG; a set whose table has overflowed refuses everything.
 * On the device (csrc/kcount.hip, kqv.hpp): one byte per slot, packed four to a 32-bit word (13 bytes a slot), allocated and zeroed at the first
 * kset_copies, freed by the seal; a byte is raised by a compare-and-swap of its word, so it never passes CN_BINS - 1 and never carries.
 * ------------------------------------------------------------------------------------------------- */
#define CORNETTO_KSET_CN_BINS 6
/* the k-mers of every contig of `a` into copies[] (kq_copies); may be called repeatedly, once per batch of a streamer.  CORNETTO_E_NOMEM: the
 * copies could not be allocated (the message says how many bytes were wanted), or the table overflowed and the set is unusable. */
int cornetto_kset_copies(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a);
/* every copy count to 0; the keys stay, assembly-only ones included */
int cornetto_kset_copies_clear(cornetto_accel_t *h, cornetto_kset_t *s);
/* spec[0 .. CORNETTO_KSET_CN_BINS * CORNETTO_KSET_HIST_BINS) and totals[0 .. 2) = {solid, found} for min_count (kq_spectrum) */
int cornetto_kset_spectrum(cornetto_accel_t *h, cornetto_kset_t *s, int32_t channel, int32_t min_count, int64_t *spec, int64_t *totals);

/* ---------------------------------------------------------------------------------------------------
 * Switch and Hamming error of a phased assembly against parental k-mers: `cornetto trioeval`.  An EXTENSION (the reference's protocol runs
 * `yak trioeval pat.yak mat.yak asm.fa` at this step, docs/protocol.md:292-308; yak works from read k-mer counts with thresholds, this works
 * from parental or truth-haplotype ASSEMBLIES, as `cornetto qv hg002.mat.fa -t hg002.pat.fa` does; parity with yak is unpinned).  THE RULE:
 *   - k, the valid bytes, the positions that hold a k-mer and the canonical code are those of `cornetto qv` above;
 *   - P: the canonical k-mers of every position of every record of the paternal input; M: the same of the maternal input;
 *   - a position of an assembly contig is a MARKER iff its k-mer is in exactly one of the two sets: of type pat when in P and not in M, of
 *     type mat when in M and not in P; a k-mer in both sets or in neither is no marker;
 *   - per contig: kmers = the positions that hold a k-mer, pat and mat = the markers of either type, all counted with multiplicity;
 *   - per contig, the four PAIR counts pp, pm, mp, mm over every marker that has a marker in front of it in the same contig: the pair is
 *     (type of the nearest marker at a smaller position, own type).  Invalid bytes between the two and their distance do not matter; no pair
 *     spans two contigs; hence pp + pm + mp + mm = max(pat + mat - 1, 0);
 *   - per assembly: switches = sum(pm + mp), pairs = sum(pp + pm + mp + mm), hamming = sum over the contigs of min(pat, mat), markers =
 *     sum(pat + mat); switch_rate = switches / pairs and hamming_rate = hamming / markers, on the host in double from the integers, printed
 *     with %.6f, or NA when the denominator is 0.
 * Every integer is independent of the order of insertion and of the probes.
 * On the device (csrc/ktrio.hip, ktrio.hpp, kqv.hpp): the table of `qv` with a 2-bit tag in bits 63:62 of a slot (bit 0 pat, bit 1 mat; every key
 * is below 2^62); a set is either plain or tagged, decided by its first add, and the calls of the other family return CORNETTO_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------------- */
#define CORNETTO_TRIO_PAT 1
#define CORNETTO_TRIO_MAT 2
#define CORNETTO_TRIO_COUNTS 7 /* per contig: kmers, pat, mat, pp, pm, mp, mm */
/* cornetto_kset_add() with a tag: CORNETTO_TRIO_PAT or CORNETTO_TRIO_MAT, any other value is CORNETTO_E_ARG.  stats as for a plain set: the
 * positions inserted and the distinct k-mers of the union.  Overflow as in cornetto_kset_add(): CORNETTO_E_NOMEM, the set is unusable, no hang. */
int cornetto_kset_add_tag(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a, int32_t tag);
/* counts[CORNETTO_TRIO_COUNTS * c + 0 .. 7) for the contigs of `a` (kt_mark, kt_tile, kt_seam).  0 contigs, contigs without a tile and contigs
 * shorter than k are accepted (all counts 0).  One call at a time per set. */
int cornetto_kset_phase(cornetto_accel_t *h, cornetto_kset_t *s, const cornetto_asm_t *a, int64_t *counts);

/* ---------------------------------------------------------------------------------------------------
 * fixasm output text: the records of a resident assembly, renamed and reoriented
 * ------------------------------------------------------------------------------------------------- */

/* One record of the text: heads[head .. head + head_len) (the ">name\n" line, built by the caller), then the bases of contig `ctg`
 * of the assembly — reversed and complemented when rc != 0, as reverse_complement() does it (src/fixasm.c:208-224: only the
 * upper-case A<->T and C<->G are complemented; lower case, N and IUPAC codes are reversed only) — then '\n'.  Concatenated
 * over the records, this is what fix_the_assembly() prints with ">%s_%d\n%s\n" (src/fixasm.c:384). */
typedef struct cornetto_emit_rec {
    int32_t ctg;
    int32_t rc;
    int64_t head;
    int64_t head_len;
} cornetto_emit_rec_t;

/* cornetto_emit_open(): a plan over `a` (which must outlive it) and recs[0..n); heads (n_heads bytes) is copied, *total_bytes is
 * the length of the whole text.  cornetto_emit_get(): bytes [at, at + n) of the text into `dst_pinned` (pinned memory:
 * cornetto_pinned_alloc), asynchronously, on queue `slot` (0..3: the kernel of a window on one slot runs beside the copy of
 * another's); a window may cut records anywhere.  cornetto_emit_wait(): returns when the last get of that slot has landed.
 * Device memory: the plan (40 B per record + the head bytes) and one slab per slot of the largest window asked of it. */
typedef struct cornetto_emit cornetto_emit_t;
int cornetto_emit_open(cornetto_accel_t *h, const cornetto_asm_t *a, const cornetto_emit_rec_t *recs, int64_t n, const char *heads,
                       int64_t n_heads, cornetto_emit_t **out, int64_t *total_bytes);
int cornetto_emit_get(cornetto_accel_t *h, cornetto_emit_t *e, char *dst_pinned, int64_t at, int64_t n, int slot);
int cornetto_emit_wait(cornetto_accel_t *h, cornetto_emit_t *e, int slot);
void cornetto_emit_free(cornetto_accel_t *h, cornetto_emit_t *e);

/* ---------------------------------------------------------------------------------------------------
 * panel interval stage — scripts/create-cornetto.sh:41-66 without bedtools / sort / awk (parity with bedtools itself
 * is unpinned: see cornetto_amd/csrc/panel.hip)
 * ------------------------------------------------------------------------------------------------- */

/* cornetto_cov_select() followed, on the device, by `bedtools merge -d merge_dist` and `awk '($3-$2)>=min_len'`
 * (create-cornetto.sh:44-47: -d 1000, 30000): the selected windows never leave the device, only the merged intervals
 * {ctg, start, finish} come back (by contig index, by start).  Release with cornetto_free(). */
int cornetto_cov_select_merged(cornetto_accel_t *h, const cornetto_cov_t *c, int32_t lo, int32_t hi, float low_mq, int32_t edge_len,
                               int32_t min_ctg_len, int boring, int32_t merge_dist, int32_t min_len, cornetto_ivl_t **ivls,
                               int64_t *n_ivls);

/* `bedtools merge -d dist` of intervals that are in (contig, start) order (CORNETTO_E_ARG if they are not), on the
 * device: an interval that starts at most `dist` past the largest finish so far in its contig is merged into it. */
int cornetto_ivl_merge(cornetto_accel_t *h, const cornetto_ivl_t *in, int64_t n, int32_t dist, cornetto_ivl_t **out, int64_t *n_out);

typedef struct {
    int32_t min_lowq_len; /* keep hifiasm "low quality" rows of at least this length (8000, create-cornetto.sh:50; 7500, recreate-cornetto.sh:35) */
    int32_t extend;       /* rows that start beyond extend_gate grow by this many bases to the LEFT (40000, :53; 40000, recreate :38) */
    int32_t edge_len;     /* add the first / last edge_len bases of every longer contig (200000, :56) */
    int32_t merge_dist;   /* bedtools merge -d (200000, :59) */
    int32_t min_ctg_len;  /* contigs shorter than this contribute nothing (800000, :65; 1000000, recreate :47) */
    int32_t extend_right; /* ... and by this many to the RIGHT (40000, :53; 50000, recreate :38) */
    int32_t extend_gate;  /* the awk's `if ($2 > gate)` (40000, :53; 50000, recreate :38) */
} cornetto_panel_opt_t;
void cornetto_panel_defaults(cornetto_panel_opt_t *opt);          /* scripts/create-cornetto.sh */
void cornetto_panel_defaults_recreate(cornetto_panel_opt_t *opt); /* scripts/recreate-cornetto.sh:34-49 (no coverage stage: n_fun = 0) */

/* Steps 4-9 of create-cornetto.sh (:50-66) on index-based intervals: fun = output of cornetto_cov_select_merged
 * (ctg = index into ctg_len, the assembly order), lowq = the rows of the hifiasm low-quality BED (any order).
 * Result: the "boring bits" before bigenough, {ctg, start, finish}, in assembly order; cornetto_free() it.  Host only. */
int cornetto_panel_boring(const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *fun, int64_t n_fun, const cornetto_ivl_t *lowq,
                          int64_t n_lowq, const cornetto_panel_opt_t *opt, cornetto_ivl_t **boring, int64_t *n_boring);

/* ---------------------------------------------------------------------------------------------------
 * haplotype stage of the diploid panel — scripts/create-hapnetto.sh:40-67 without cut / sort / awk / bedtools, on the
 * device (parity with bedtools itself is unpinned: see cornetto_amd/csrc/hap.hip)
 * ------------------------------------------------------------------------------------------------- */

/* one line of a haplotype-to-primary PAF as the script reads it (scripts/create-hapnetto.sh:44,50): column 1 as an id that
 * is only compared for equality within its haplotype, column 6 as an index into the assembly BED, columns 8 and 9 */
typedef struct {
    int32_t query, ctg, start, finish;
} cornetto_hap_row_t;

typedef struct {
    int32_t merge_dist; /* bedtools merge -d within one (query, target) pair (1000000, scripts/create-hapnetto.sh:50) */
    int32_t flank;      /* half width of a corner (500, scripts/create-hapnetto.sh:58) */
} cornetto_hap_opt_t;
void cornetto_hap_defaults(cornetto_hap_opt_t *opt);

/* The merged haplotype funbits (hap1_hap2_funbits.bed, scripts/create-hapnetto.sh:67) of n_hap haplotypes.  rows: the rows of
 * haplotype 0, then of haplotype 1, ... in any order, n_rows[k] of haplotype k.  Per haplotype: blocks = merge -d merge_dist of
 * the rows of every (query, target) pair on its own (scripts/create-hapnetto.sh:48-51; a gap of exactly merge_dist merges);
 * gaps = every contig [0, len) minus the union of the blocks on it (scripts/create-hapnetto.sh:55; a contig without blocks is
 * one gap, a contig of length 0 none); corners = [start - flank, start + flank) of every block with start >= flank and
 * [finish - flank, finish + flank) of every block with finish >= flank, not clamped to the contig, capped at INT32_MAX
 * (scripts/create-hapnetto.sh:58); funbits = merge of gaps and corners, overlapping and book-ended rows merge
 * (scripts/create-hapnetto.sh:61).  Result: the merge of the funbits of all haplotypes (scripts/create-hapnetto.sh:67),
 * by (ctg, start); it joins the `fun` rows of cornetto_panel_boring() (scripts/create-hapnetto.sh:71).  A haplotype without
 * rows yields every contig as a gap.  CORNETTO_E_ARG: ctg outside [0, n_ctg), finish <= start, start < 0, a negative count or
 * length.  Release fun with cornetto_free(). */
int cornetto_hap_fun(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_hap_row_t *rows, const int64_t *n_rows,
                     int32_t n_hap, const cornetto_hap_opt_t *opt, cornetto_ivl_t **fun, int64_t *n_fun);

/* ---------------------------------------------------------------------------------------------------
 * telobreaks — src/telomere_breaks.c:47-172 (the consumer of the sdust BED and the telofind TSV)
 * ------------------------------------------------------------------------------------------------- */

/* one row of the telofind TSV as telobreaks reads it (:97): contig, start, end, matched length (6th column) */
typedef struct {
    int32_t ctg, start, end, matched;
} cornetto_telrow_t;

/* The bitset stage of telobreaks (:79-148) for contigs given by index (the caller resolves the names; rows of names
 * that are not in the lens file are dropped, as the reference does at :83,:100: give them ctg = -1).
 * sd: low-complexity intervals [start, finish), any order, may overlap or touch.  tel: telofind rows; those with
 * matched < 24 are ignored (MIN_TEL, :10,:98).  out[] = the numbers the reference prints (:140-142): for every maximal
 * run of the low-complexity bitset that contains a telomere row together with its 100-base flanks (clipped to the
 * contig): {ctg, first position - 1 clamped at 0, last position}, by contig index, then by position.
 * The reference prints contigs in khash bucket order: cornetto_khash_str_order().  An sd interval that ends beyond its contig
 * is cut at the contig's end: sdust itself prints such intervals for a low-complexity run at the end of a contig (up to W
 * beyond the last base), the reference sets those bits beyond its bitset (:85) and never reads them (:103,:118,:136).  Other
 * coordinates outside the contig (a negative start, a telomere row beyond the end) are unchecked heap indices in the reference;
 * here they are CORNETTO_E_FORMAT.  Release out with cornetto_free(). */
int cornetto_telobreaks(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *sd, int64_t n_sd,
                        const cornetto_telrow_t *tel, int64_t n_tel, cornetto_ivl_t **out, int64_t *n_out);

/* The telomere breaks of a resident assembly: sdust(T, W) and telofind(motif) on the device, then the interval rule below; equal to
 * cornetto_sdust_asm() + cornetto_telofind() + cornetto_telobreaks() on their results (rows {ctg, start, end, end - start}), i.e. to
 * the chain of test/realtest.sh:65-69 (`cornetto sdust` and `cornetto telofind` each write a file, `cornetto telobreaks` reads both and
 * the table of lengths) with src/telomere_breaks.c:79-148 behind it.
 * Neither list leaves the device.  T, W: the limits of cornetto_sdust_asm(); motif: those of cornetto_telofind().  rows by contig, then
 * by start; release them with cornetto_free(). */
int cornetto_telo_breaks(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, int32_t T, int32_t W,
                         cornetto_ivl_t **rows, int64_t *n_rows);

/* The same kernels on explicit lists: src/telomere_breaks.c:95-148 as a rule on intervals instead of two bitsets.  sd must be sorted by
 * (ctg, start), with every start greater than the previous finish in the same contig (what sdust prints: src/sdust/sdust.c:88-102 merges
 * an interval that starts at or before the previous finish); a list that is not, or that names a contig outside [0, n_ctg):
 * CORNETTO_E_ARG, checked on the device.  finish may exceed the contig length (it is cut there, as cornetto_telobreaks() cuts it).  Then a
 * row of tel with matched >= 24 marks the one interval that contains [max(0, start - 100), min(L, end + 100)), and every marked interval
 * comes out once as {ctg, max(start - 1, 0), min(finish, L) - 1}: the records of cornetto_telobreaks() in the same order.  Rows of a
 * contig outside [0, n_ctg) are dropped; a row outside its contig or with start >= end, or an interval with a negative start:
 * CORNETTO_E_FORMAT, as there.  As there, too: with an empty sd or an empty tel nothing can be marked, and the rows are not looked at
 * (an empty sd: no kernel runs; an empty tel: sd is still checked); an interval that starts at or beyond its contig's end is empty after
 * the cut and marks nothing, without an error.  At most 2^31 - 1 intervals.  Release out with cornetto_free(). */
int cornetto_telobreaks_ivl(cornetto_accel_t *h, const int32_t *ctg_len, int32_t n_ctg, const cornetto_ivl_t *sd, int64_t n_sd,
                            const cornetto_telrow_t *tel, int64_t n_tel, cornetto_ivl_t **out, int64_t *n_out);

/* Host helper: the iteration order of the reference's khash string map (klib khash 0.2.8, src/khash.h) after
 * kh_put() of names[0..n) in that order — the order in which telobreaks prints its contigs (:133).  slot[i] = dense
 * id of the distinct key of names[i] (ids in order of first appearance); order[k] = id in the k-th occupied bucket.
 * Returns the number of distinct keys, -1 on a bad argument.  Needs no device. */
int32_t cornetto_khash_str_order(const char *const *names, int32_t n, int32_t *slot, int32_t *order);

#ifdef __cplusplus
}
#endif
#endif /* CORNETTO_ACCEL_H */
