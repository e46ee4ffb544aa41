/* fqseq.c — `seq --fastq FILE [-m INT] [--bgzf]` (not in the reference): the text `seq` prints, written on the device (cornetto_fqseq_*;
 * include/cornetto_accel.h states the rules).  cli/bam.c's window / slab loop over the feeds of cli/bgcomp.c:
 *   a BGZF file (told by its first bytes, cli_depth_kind)   the compressed bytes cross the bus slab by slab (cli_bgz_*), the host walks the
 *                                                           chain, the blocks are fed and inflated on the device;
 *   everything else                                         plain text, another gzip, a FIFO, BGZF under $CORNETTO_BGZF=0: gzread() into a
 *                                                           pinned piece of $CORNETTO_FASTQ_PIECE bytes, fed as plain bytes.
 * The window's text is pulled in slabs of $CORNETTO_EMIT_SLAB bytes on the four copy slots, to stdout or as BGZF members under --bgzf.  Where
 * the device stops — a group of lines that is no plain record, or a record larger than the window ($CORNETTO_FASTQ_WINDOW) — the sequential
 * reader of cli/fastx.c goes on at cornetto_fqseq_rest(): behind the bytes gzread() has handed over already, or in the BGZF file opened again
 * with gzopen() and gzseek().  None of the three environment variables changes a byte of the output. */
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "cli.h"

static int64_t fqs_env(const char *name, int64_t dflt, int64_t min, int64_t max)
{
    const char *e = getenv(name);
    if (!e) return dflt;
    char *end = NULL;
    const long long v = strtoll(e, &end, 10);
    if (end == e || *end || v < min || v > max) {
        CLI_ERROR("%s wants a number of bytes from %lld to %lld. Found %s", name, (long long)min, (long long)max, e);
        exit(EXIT_FAILURE);
    }
    return v;
}

static void fqs_trace(const char *what, double seconds)
{
    if (getenv("CORNETTO_CLI_TRACE")) fprintf(stderr, "[cli trace] seq --fastq: %s %.3f s\n", what, seconds);
}

/* the four copy slots and their pinned buffers (allocated when a slot is first used: a small file takes one) */
typedef struct {
    cornetto_accel_t *h;
    cornetto_fqseq_t *q;
    int bgzf;
    int64_t slab_bytes, pin_bytes;
    char *pin[4];
    double t_text;
} fqs_out_t;

/* the window's text, a slab at a time: the kernel of one slab runs beside the copies of the others and beside the write of the one before */
static void fqs_pull(fqs_out_t *o, int64_t n_text)
{
    const double t0 = cli_realtime();
    int64_t at = 0, len[4] = {0, 0, 0, 0};
    for (int k = 0; at < n_text || len[0] || len[1] || len[2] || len[3]; ++k) {
        const int s = k & 3;
        if (len[s] && o->bgzf) {
            int64_t n_comp = 0;
            cli_accel_check(o->h, cornetto_fqseq_wait_bgzf(o->h, o->q, s, &n_comp), "FASTQ text");
            cli_bgzf_out_members(o->pin[s], (size_t)n_comp);
            len[s] = 0;
        } else if (len[s]) {
            cli_accel_check(o->h, cornetto_fqseq_wait(o->h, o->q, s), "FASTQ text");
            if (fwrite(o->pin[s], 1, (size_t)len[s], stdout) != (size_t)len[s]) {
                CLI_ERROR("%s", "cannot write to the standard output");
                exit(EXIT_FAILURE);
            }
            len[s] = 0;
        }
        if (at < n_text) {
            if (!o->pin[s] && !(o->pin[s] = (char *)cornetto_pinned_alloc((size_t)o->pin_bytes))) {
                CLI_ERROR("%s", "cannot allocate the pinned output buffers");
                exit(EXIT_FAILURE);
            }
            len[s] = n_text - at < o->slab_bytes ? n_text - at : o->slab_bytes;
            if (o->bgzf) cli_accel_check(o->h, cornetto_fqseq_get_bgzf(o->h, o->q, o->pin[s], o->pin_bytes, at, len[s], s), "FASTQ text");
            else cli_accel_check(o->h, cornetto_fqseq_get(o->h, o->q, o->pin[s], at, len[s], s), "FASTQ text");
            at += len[s];
        }
    }
    o->t_text += cli_realtime() - t0;
}

/* one feed and its text -> the status: CORNETTO_OK, CORNETTO_E_FORMAT (a damaged block; the text in front of it is out) or CORNETTO_E_NOMEM with
 * nothing taken (a record larger than the window) */
static int fqs_feed(fqs_out_t *o, const cornetto_bgsrc_t *src, int final, int64_t *taken, int32_t *plain, double *t_feed)
{
    int64_t n_text = 0;
    const double t0 = cli_realtime();
    const int rc = cornetto_fqseq_feed(o->h, o->q, src, final, taken, &n_text, plain);
    *t_feed += cli_realtime() - t0;
    if (rc == CORNETTO_E_NOMEM && *taken == 0) return rc;
    if (rc != CORNETTO_OK && rc != CORNETTO_E_FORMAT) cli_accel_check(o->h, rc, "FASTQ text");
    fqs_pull(o, n_text);
    return rc;
}

void cli_fastq_seq(cornetto_accel_t *h, const char *path, int min_len, uint64_t stats[4])
{
    const double t_start = cli_realtime();
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        CLI_ERROR("Could not to open file %s: %s", path, strerror(errno)); /* F_CHK, src/error.h:114-119: its words */
        exit(EXIT_FAILURE);
    }
    const int kind = cli_depth_kind(fp);
    const int on_device = kind == 1 && !(getenv("CORNETTO_BGZF") && !atoi(getenv("CORNETTO_BGZF")));
    cornetto_fqseq_opt_t opt;
    cornetto_fqseq_defaults(&opt);
    opt.min_len = min_len;
    opt.window = fqs_env("CORNETTO_FASTQ_WINDOW", opt.window, 1, 0xFFFFFF00ll);
    fqs_out_t o;
    memset(&o, 0, sizeof(o));
    o.h = h;
    o.bgzf = cli_bgzf_out_active();
    o.slab_bytes = fqs_env("CORNETTO_EMIT_SLAB", 32ll << 20, 1, 1ll << 30);
    o.pin_bytes = o.bgzf ? (o.slab_bytes + 65279) / 65280 * 65536 : o.slab_bytes;
    (void)cornetto_accel_set_timing(h, 0);      /* (nobody reads the kernel times here: no event packets beside the kernels) */
    cli_accel_check(h, cornetto_fqseq_open(h, &opt, &o.q), "FASTQ text");
    if (cli_qmean_max_err() >= 0) cli_accel_check(h, cornetto_fqseq_set_max_err(h, o.q, cli_qmean_max_err()), "FASTQ text");
    double t_read = 0, t_feed = 0;
    int32_t plain = 1;
    int nomem = 0;
    cli_fastx_t *fx = NULL;      /* the sequential reader, where the device has stopped */
    char *buf = NULL;            /* the pinned piece of the gzread() feed */
    if (on_device) {
        int64_t slab = opt.window / 4 > (1ll << 20) ? opt.window / 4 : 1ll << 20;
        if (slab > (64ll << 20)) slab = 64ll << 20;
        cli_bgz_t *z = cli_bgz_open(h, path, fileno(fp), slab, 8);
        for (int last = 0; !last && plain && !nomem;) {
            cornetto_bgsrc_t src;
            double t0 = cli_realtime();
            (void)cli_bgz_next(h, z, opt.window, &src, &last);
            t_read += cli_realtime() - t0;
            for (int64_t i = 0; (i < src.n_blocks || (src.n_blocks == 0 && last)) && plain && !nomem;) {
                cornetto_bgsrc_t part = src;
                part.blocks = src.blocks + i;
                part.n_blocks = src.n_blocks - i;
                int64_t taken = 0;
                const int rc = fqs_feed(&o, &part, last, &taken, &plain, &t_feed);
                if (rc == CORNETTO_E_FORMAT) {      /* the text of the records in front of the block is out; no summary, no end-of-file block */
                    fflush(stdout);
                    cli_bgz_fail_block(z, (long long)cornetto_fqseq_error(o.q));
                }
                if (rc == CORNETTO_E_NOMEM) nomem = 1;
                i += taken;
                if (src.n_blocks == 0) break;
            }
        }
        cli_bgz_close(h, z);
        if (!plain || nomem) {
            gzFile gz = (gzFile)cli_gz_open(path, 1);
            if (gzseek(gz, (z_off_t)cornetto_fqseq_rest(o.q), SEEK_SET) < 0) {
                CLI_ERROR("reading %s failed", path);
                exit(EXIT_FAILURE);
            }
            fx = cli_fastx_open_prefixed(gz, NULL, 0);
        }
    } else {
        gzFile gz = gzdopen(dup(fileno(fp)), "r");      /* (the one open of a FIFO) */
        if (!gz) {
            CLI_ERROR("Could not to open file %s: %s", path, strerror(errno));
            exit(EXIT_FAILURE);
        }
        gzbuffer(gz, 1 << 18);
        const int64_t piece = fqs_env("CORNETTO_FASTQ_PIECE", 64ll << 20, 1, 0xF0000000ll);
        /* buf: the bytes of the stream from the device's last whole record on — `tail` bytes read earlier, then the new piece */
        int64_t cap = piece, tail = 0, got = 0, read_total = 0;
        buf = (char *)cornetto_pinned_alloc((size_t)cap);
        for (int eof = 0; buf && !eof && plain && !nomem;) {
            if (tail + piece > cap) {      /* (a record longer than a piece) */
                cap = tail + piece + tail / 2;
                char *nb = (char *)cornetto_pinned_alloc((size_t)cap);
                if (nb) memcpy(nb, buf, (size_t)tail);
                cornetto_pinned_free(buf);
                buf = nb;
                if (!buf) break;
            }
            double t0 = cli_realtime();
            for (got = 0; got < piece;) {
                const int64_t ask = piece - got > (1 << 30) ? (1 << 30) : piece - got;
                const int r = gzread(gz, buf + tail + got, (unsigned)ask);
                if (r < 0) {
                    CLI_ERROR("reading %s failed", path);
                    exit(EXIT_FAILURE);
                }
                got += r;
                if (r < ask) {
                    eof = 1;
                    break;
                }
            }
            t_read += cli_realtime() - t0;
            read_total += got;
            for (int64_t at = 0, first = 1; (at < got || (first && eof)) && plain && !nomem; first = 0) {
                const cornetto_bgsrc_t src = {buf + tail + at, got - at, NULL, NULL, 0};
                int64_t taken = 0;
                if (fqs_feed(&o, &src, eof, &taken, &plain, &t_feed) == CORNETTO_E_NOMEM) nomem = 1;
                at += taken;
            }
            /* what no record of the device's holds yet stays in front of the next piece */
            const int64_t keep = read_total - cornetto_fqseq_rest(o.q);
            if (keep < 0 || keep > tail + got) {
                CLI_ERROR("%s", "the device consumed bytes it was not given");
                exit(EXIT_FAILURE);
            }
            memmove(buf, buf + tail + got - keep, (size_t)keep);
            tail = keep;
        }
        if (!buf) {
            CLI_ERROR("%s", "cannot allocate the pinned read buffer");
            exit(EXIT_FAILURE);
        }
        if (!plain || nomem) fx = cli_fastx_open_prefixed(gz, buf, (size_t)tail);      /* (the bytes gzread() has handed over first; buf lives until the reader is closed) */
        else gzclose(gz);
    }
    int64_t st[5] = {0, 0, 0, 0, 0};
    cornetto_fqseq_stats(o.q, st);
    for (int k = 0; k < 4; ++k) stats[k] += (uint64_t)st[k];
    int64_t qst[2] = {0, 0};
    cornetto_fqseq_qstats(o.q, qst);      /* (what the device printed; the sequential reader below counts its own) */
    cli_qmean_add(qst[0], qst[1]);
    if (fx) {
        if (nomem)
            CLI_WARNING("%s: a record does not fit the window of %lld bytes%s (CORNETTO_FASTQ_WINDOW): reading the rest of the file on the host, one thread", path,
                        (long long)opt.window, on_device ? " with one more block" : "");
        cli_seq_records(fx, min_len, stats);
        cli_fastx_close(fx);
    }
    fqs_trace("read", t_read);
    fqs_trace("feed (inflate, index, frame, size, scan)", t_feed);
    fqs_trace("text (kernel, copy, write)", o.t_text);
    fqs_trace("all", cli_realtime() - t_start);
    cornetto_fqseq_close(h, o.q);
    for (int s = 0; s < 4; ++s) cornetto_pinned_free(o.pin[s]);
    cornetto_pinned_free(buf);
    fclose(fp);
}
