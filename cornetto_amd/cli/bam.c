/* bam.c — `(no)boringbits --bam FILE`: both coverage tracks from the BAM on the device, and `seq --bam FILE [--bgzf]`: its FASTQ text (extensions;
 * include/cornetto_accel.h states the rules of both; they share the reader below and differ in the object they feed).
 * The compressed file is read a chunk at a time into ONE pinned slab (no ring, no reader thread yet: read, upload and kernels follow
 * each other); the host walks the BGZF chain of the chunk
 * (cornetto_bgzf_scan), finds the header by inflating the leading blocks with zlib (cornetto_bam_header) and hands the chunk's blocks to
 * cornetto_bamdepth_feed(), which inflates them a window at a time, frames the records and walks their CIGARs.  The bytes behind the last
 * whole block of a chunk open the next chunk.  $CORNETTO_BAM_WINDOW: bytes of inflated BAM per window (an operating parameter: it never
 * changes a result; a record that does not fit sends the file to the host reader). */
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "cli.h"

static void bam_device_fail(cornetto_accel_t *h, const char *path, cornetto_bamdepth_t *b, int rc)
{
    if (rc == CORNETTO_E_FORMAT) {
        const cornetto_bamerr_t *e = cornetto_bamdepth_error(b);
        if (e && e->kind) cli_bam_fail(path, e->kind, (long long)e->record, e->a, e->b);
    }
    cli_accel_check(h, rc, "BAM ingest");
}

/* the bytes of block b of the slab, appended to *hdr (zlib's raw inflate) -> 0, or -1 when the block is not what its footer says */
static int bam_inflate_block(const uint8_t *slab, const cornetto_bgzf_block_t *b, uint8_t **hdr, int64_t *n_hdr, int64_t *cap_hdr)
{
    if (*n_hdr + b->n_dst >= *cap_hdr) {
        *cap_hdr = (*n_hdr + b->n_dst) * 2 + 65536;
        *hdr = (uint8_t *)cli_xrealloc(*hdr, (size_t)*cap_hdr);
    }
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return -1;
    z.next_in = (Bytef *)(slab + b->src);
    z.avail_in = (uInt)b->n_src;
    z.next_out = *hdr + *n_hdr;
    z.avail_out = (uInt)b->n_dst;
    const int zr = b->n_dst > 0 || b->n_src > 0 ? inflate(&z, Z_FINISH) : Z_STREAM_END;
    const int ok = zr == Z_STREAM_END && (int64_t)z.total_out == b->n_dst && (uint32_t)crc32(crc32(0L, Z_NULL, 0), *hdr + *n_hdr, (uInt)b->n_dst) == b->crc;
    inflateEnd(&z);
    if (!ok) return -1;
    *n_hdr += b->n_dst;
    return 0;
}

/* ---- the reader both users share: the compressed file a chunk at a time into ONE pinned slab, the BGZF chain of the chunk walked on the
 * host, the header found by inflating the leading blocks with zlib; the bytes behind the last whole block of a chunk open the next one ---- */
typedef struct {
    FILE *fp;
    const char *path;
    int64_t chunk, cap_blocks, file_off, pend, dst;
    uint8_t *slab, *hdr;
    cornetto_bgzf_block_t *blocks;
    cornetto_text_t *comp;
    int64_t n_hdr, cap_hdr, hdr_blocks;
    int eof, have_header;
    int32_t n_ref, *ref_len;
    char **ref_name;
} bam_reader_t;

/* $CORNETTO_BAM_WINDOW, or the default */
static int64_t bam_window_env(int64_t dflt, int64_t max)
{
    if (!getenv("CORNETTO_BAM_WINDOW")) return dflt;
    char *end = NULL;
    const long long w = strtoll(getenv("CORNETTO_BAM_WINDOW"), &end, 10);
    if (end == getenv("CORNETTO_BAM_WINDOW") || *end || w < 1 || w > max) {
        CLI_ERROR("CORNETTO_BAM_WINDOW wants a number of bytes from 1 to %lld. Found %s", (long long)max, getenv("CORNETTO_BAM_WINDOW"));
        exit(EXIT_FAILURE);
    }
    return w;
}

static void bam_reader_open(cornetto_accel_t *h, bam_reader_t *r, const char *path, int64_t window)
{
    memset(r, 0, sizeof(*r));
    r->path = path;
    r->fp = fopen(path, "rb");
    if (!r->fp) {
        CLI_ERROR("Failed to open %s : No such file or directory.", path);
        exit(EXIT_FAILURE);
    }
    int64_t chunk = window > (1ll << 20) ? window : 1ll << 20;      /* compressed bytes per feed: a feed fills a window whatever the ratio */
    if (chunk > (1ll << 30)) chunk = 1ll << 30;
    if (fseek(r->fp, 0, SEEK_END) == 0) {      /* (a small file: a small slab) */
        const int64_t size = (int64_t)ftell(r->fp);
        if (size >= 0 && size + 65536 < chunk) chunk = size + 65536;
        rewind(r->fp);
    }
    r->chunk = chunk;
    r->slab = (uint8_t *)cornetto_pinned_alloc((size_t)chunk);
    r->cap_blocks = chunk / 26 + 1;
    r->blocks = (cornetto_bgzf_block_t *)cli_xmalloc((size_t)r->cap_blocks * sizeof(cornetto_bgzf_block_t));
    if (!r->slab) {
        CLI_ERROR("%s", "cannot allocate the pinned read buffer");
        exit(EXIT_FAILURE);
    }
    cli_accel_check(h, cornetto_text_open(h, chunk, &r->comp), "BAM ingest");
}

/* The next chunk: its whole blocks (r->blocks[0 .. *nb), src counted from the chunk's first byte) are on the device in r->comp.  The chunk in
 * which the header ends: *skip = the header's bytes, and n_ref / ref_name / ref_len are set.  -> 0: the file has ended, nothing was read */
static int bam_reader_next(cornetto_accel_t *h, bam_reader_t *r, int64_t *nb_out, int64_t *skip)
{
    *nb_out = 0;
    *skip = 0;
    if (r->eof) return 0;
    const size_t want = (size_t)(r->chunk - r->pend), got = fread(r->slab + r->pend, 1, want, r->fp);
    r->eof = got < want;
    const int64_t n = r->pend + (int64_t)got;
    int64_t nb = 0, resume = r->file_off;
    int32_t broken = 0;
    cli_accel_check(h, cornetto_bgzf_scan(r->slab, n, r->file_off, &r->dst, r->blocks, r->cap_blocks, &nb, &resume, &broken), "BGZF chain");
    const int64_t used = resume - r->file_off;
    if (broken || (r->eof && used < n) || (!r->eof && used == 0)) cli_bam_fail(r->path, r->have_header ? 6 : 7, 0, 0, 0);
    for (int64_t i = 0; i < nb; ++i) r->blocks[i].src -= r->file_off;
    if (!r->have_header) {       /* the header: as many leading blocks as it takes */
        int rc = 1;
        while (rc == 1 && r->hdr_blocks < nb) {
            if (bam_inflate_block(r->slab, &r->blocks[r->hdr_blocks++], &r->hdr, &r->n_hdr, &r->cap_hdr) != 0) cli_bam_fail(r->path, 6, 0, 0, 0);
            int64_t hb = 0;
            rc = cornetto_bam_header(r->hdr, r->n_hdr, &r->n_ref, &r->ref_name, &r->ref_len, &hb);
            *skip = hb;
        }
        if (rc == 1 && r->eof) cli_bam_fail(r->path, 2, -1, 0, -1);
        if (rc == 1) {
            CLI_ERROR("%s: a BAM header of more than %lld compressed bytes", r->path, (long long)r->chunk);
            exit(EXIT_FAILURE);
        }
        if (rc != CORNETTO_OK) cli_bam_fail(r->path, 7, -1, 0, 0);
        r->have_header = 1;
    }
    if (used > 0) cli_accel_check(h, cornetto_text_put(h, r->comp, (const char *)r->slab, used, 0, 0), "BAM upload");
    *nb_out = nb;
    r->pend = n - used;
    r->file_off = resume;
    return 1;
}

/* the chunk's bytes behind its last whole block move to the slab's front: after the chunk's blocks have been fed (the put reads the slab) */
static void bam_reader_advance(bam_reader_t *r, int64_t used_before)
{
    if (r->pend > 0) memmove(r->slab, r->slab + used_before, (size_t)r->pend);
}

/* (the contig names and lengths stay with the caller) */
static void bam_reader_close(cornetto_accel_t *h, bam_reader_t *r)
{
    fclose(r->fp);
    free(r->hdr);
    free(r->blocks);
    cornetto_text_free(h, r->comp);
    cornetto_pinned_free(r->slab);
}

static void bam_reader_free_refs(bam_reader_t *r)
{
    for (int32_t i = 0; i < r->n_ref; ++i) free(r->ref_name[i]);
    free(r->ref_name);
    free(r->ref_len);
    r->ref_name = NULL;
    r->ref_len = NULL;
}

int cli_bam_ingest(cornetto_accel_t *h, const char *path, int min_mapq, cornetto_cov_t **cov, int32_t *n_ctg, char ***names, int64_t *n_clamped)
{
    cornetto_bamdepth_opt_t opt;
    cornetto_bamdepth_defaults(&opt);
    opt.min_mapq = min_mapq;
    opt.window = bam_window_env(opt.window, 0xF0000000ll);
    bam_reader_t R;
    bam_reader_open(h, &R, path, opt.window);
    cornetto_bamdepth_t *b = NULL;
    int nomem = 0;
    int64_t nb = 0, skip = 0;
    for (;;) {
        const int64_t file_off = R.file_off;
        if (!bam_reader_next(h, &R, &nb, &skip)) break;
        if (!b) {
            const int rc = cornetto_bamdepth_open(h, &opt, R.ref_len, R.n_ref, &b);
            if (rc == CORNETTO_E_NOMEM) {
                nomem = 2;
                break;
            }
            cli_accel_check(h, rc, "BAM ingest");
        }
        const int rc = cornetto_bamdepth_feed(h, b, R.comp, R.blocks, nb, skip);
        if (rc == CORNETTO_E_NOMEM) {
            nomem = 1;
            break;
        }
        if (rc != CORNETTO_OK) bam_device_fail(h, path, b, rc);
        bam_reader_advance(&R, R.file_off - file_off);
    }
    int32_t n_ref = R.n_ref, *ref_len = R.ref_len;
    char **ref_name = R.ref_name;
    int rc = CORNETTO_OK;
    cornetto_cov_t *c = NULL;
    if (!nomem) {
        if (!b) cli_bam_fail(path, 2, -1, 0, -1);      /* (an empty file) */
        rc = cornetto_bamdepth_finish(h, b, &c, NULL, NULL, n_clamped);
        if (rc == CORNETTO_E_NOMEM) nomem = 2;
        else if (rc != CORNETTO_OK) bam_device_fail(h, path, b, rc);
    }
    cornetto_bamdepth_close(h, b);
    bam_reader_close(h, &R);
    if (nomem) {
        if (nomem == 1)
            CLI_WARNING("%s: a record does not fit the window of %lld bytes with one more block (CORNETTO_BAM_WINDOW): reading the file on the host, one thread",
                        path, (long long)opt.window);
        else
            CLI_WARNING("%s: the device has no room for the depth arrays of the %d contigs of the header: reading the file on the host, one thread", path, n_ref);
        bam_reader_free_refs(&R);
        return 1;
    }
    /* a contig without positions has no line in a per-base bedgraph: it is not a contig of the result */
    int32_t *keep = (int32_t *)cli_xmalloc(((size_t)n_ref + 1) * sizeof(int32_t)), n_keep = 0;
    for (int32_t i = 0; i < n_ref; ++i) {
        if (ref_len[i] > 0) {
            ref_name[n_keep] = ref_name[i];
            keep[n_keep++] = i;
        } else {
            free(ref_name[i]);
        }
    }
    if (n_keep < n_ref) {
        cornetto_cov_t *c2 = NULL;
        cli_accel_check(h, cornetto_cov_shard(h, c, h, keep, n_keep, &c2), "BAM ingest");
        cornetto_cov_free(h, c);
        c = c2;
    }
    free(keep);
    free(ref_len);
    *cov = c;
    *n_ctg = n_keep;
    *names = ref_name;
    return 0;
}

/* ---- `seq --bam FILE`: the FASTQ text of the BAM on the device (cornetto_bamfq_*) ---- */
static void fq_trace(const char *what, double seconds)
{
    if (getenv("CORNETTO_CLI_TRACE")) fprintf(stderr, "[cli trace] seq --bam: %s %.3f s\n", what, seconds);
}

int cli_bam_fastq(cornetto_accel_t *h, const char *path, int min_len, int duplex, uint64_t stats[4], int64_t *n_done)
{
    const double t_start = cli_realtime();
    cornetto_bamfq_opt_t opt;
    cornetto_bamfq_defaults(&opt);
    opt.min_len = min_len;
    opt.duplex = duplex;
    opt.window = bam_window_env(opt.window, 0x80000000ll);
    int64_t slab_bytes = 32ll << 20;
    if (getenv("CORNETTO_EMIT_SLAB")) {
        char *end = NULL;
        const long long v = strtoll(getenv("CORNETTO_EMIT_SLAB"), &end, 10);
        if (end == getenv("CORNETTO_EMIT_SLAB") || *end || v < 1 || v > (1ll << 30)) {
            CLI_ERROR("CORNETTO_EMIT_SLAB wants a number of bytes from 1 to %lld. Found %s", 1ll << 30, getenv("CORNETTO_EMIT_SLAB"));
            exit(EXIT_FAILURE);
        }
        slab_bytes = v;
    }
    (void)cornetto_accel_set_timing(h, 0);      /* (nobody reads the kernel times here: no event packets beside the kernels) */
    bam_reader_t R;
    bam_reader_open(h, &R, path, opt.window);
    /* --bgzf: the slab's text is deflated on the device, its members come back: 64 KiB of room for every 65280 bytes of text */
    const int bgzf = cli_bgzf_out_active();
    const int64_t pin_bytes = bgzf ? (slab_bytes + 65279) / 65280 * 65536 : slab_bytes;
    char *pin[2] = {(char *)cornetto_pinned_alloc((size_t)pin_bytes), (char *)cornetto_pinned_alloc((size_t)pin_bytes)};
    if (!pin[0] || !pin[1]) {
        CLI_ERROR("%s", "cannot allocate the pinned output buffers");
        exit(EXIT_FAILURE);
    }
    cornetto_bamfq_t *b = NULL;
    int nomem = 0, failed = CORNETTO_OK;
    int64_t nb = 0, skip = 0;
    double t_read = 0, t_feed = 0, t_text = 0;
    while (!nomem && failed == CORNETTO_OK) {
        const int64_t file_off = R.file_off;
        double t0 = cli_realtime();
        if (!bam_reader_next(h, &R, &nb, &skip)) break;
        t_read += cli_realtime() - t0;
        if (!b) {
            opt.n_ref = R.n_ref;
            cli_accel_check(h, cornetto_bamfq_open(h, &opt, &b), "BAM to FASTQ");
            if (cli_qmean_max_err() >= 0) cli_accel_check(h, cornetto_bamfq_set_max_err(h, b, cli_qmean_max_err()), "BAM to FASTQ");
        }
        for (int64_t i = 0; (i < nb || skip > 0) && !nomem && failed == CORNETTO_OK;) {
            int64_t taken = 0, n_text = 0;
            t0 = cli_realtime();
            const int rc = cornetto_bamfq_feed(h, b, R.comp, R.blocks + i, nb - i, skip, &taken, &n_text);
            t_feed += cli_realtime() - t0;
            if (rc == CORNETTO_E_NOMEM && taken == 0) {
                nomem = 1;
                break;
            }
            if (rc != CORNETTO_OK && rc != CORNETTO_E_FORMAT) cli_accel_check(h, rc, "BAM to FASTQ");
            failed = rc;
            skip = 0;
            i += taken;
            /* the window's text, a slab at a time: the kernel of one slab runs beside the copy of the other, and beside the write of the one before */
            t0 = cli_realtime();
            int64_t at = 0, len[2] = {0, 0};
            for (int k = 0; at < n_text || len[0] || len[1]; ++k) {
                const int s = k & 1;
                if (len[s] && bgzf) {
                    int64_t n_comp = 0;
                    cli_accel_check(h, cornetto_bamfq_wait_bgzf(h, b, s, &n_comp), "BAM to FASTQ");
                    cli_bgzf_out_members(pin[s], (size_t)n_comp);
                    len[s] = 0;
                } else if (len[s]) {
                    cli_accel_check(h, cornetto_bamfq_wait(h, b, s), "BAM to FASTQ");
                    if (fwrite(pin[s], 1, (size_t)len[s], stdout) != (size_t)len[s]) {
                        CLI_ERROR("%s", "cannot write to the standard output");
                        exit(EXIT_FAILURE);
                    }
                    len[s] = 0;
                }
                if (at < n_text) {
                    len[s] = n_text - at < slab_bytes ? n_text - at : slab_bytes;
                    if (bgzf) cli_accel_check(h, cornetto_bamfq_get_bgzf(h, b, pin[s], pin_bytes, at, len[s], s), "BAM to FASTQ");
                    else cli_accel_check(h, cornetto_bamfq_get(h, b, pin[s], at, len[s], s), "BAM to FASTQ");
                    at += len[s];
                }
            }
            t_text += cli_realtime() - t0;
            if (nb == 0) break;
        }
        bam_reader_advance(&R, R.file_off - file_off);
    }
    if (!nomem && failed == CORNETTO_OK) {
        if (!b) cli_bam_fail(path, 2, -1, 0, -1);      /* (an empty file) */
        failed = cornetto_bamfq_finish(h, b);
        if (failed != CORNETTO_OK && failed != CORNETTO_E_FORMAT) cli_accel_check(h, failed, "BAM to FASTQ");
    }
    int64_t st[5] = {0, 0, 0, 0, 0};
    cornetto_bamerr_t err;
    memset(&err, 0, sizeof(err));
    if (b) {
        cornetto_bamfq_stats(b, st);
        int64_t qst[2] = {0, 0};
        cornetto_bamfq_qstats(b, qst);      /* (what the device printed; the host reader counts what it prints behind it) */
        cli_qmean_add(qst[0], qst[1]);
        err = *cornetto_bamfq_error(b);
    }
    for (int k = 0; k < 4; ++k) stats[k] = (uint64_t)st[k];
    *n_done = st[4];
    fq_trace("read, chain, upload", t_read);
    fq_trace("feed (inflate, frame, size, scan)", t_feed);
    fq_trace("text (kernel, copy, write)", t_text);
    fq_trace("all", cli_realtime() - t_start);
    if (failed == CORNETTO_E_FORMAT) {
        fflush(stdout);
        if (err.kind) cli_bam_fail(path, err.kind, (long long)err.record, err.a, err.b);
        cli_accel_check(h, failed, "BAM to FASTQ");
    }
    cornetto_bamfq_close(h, b);
    bam_reader_close(h, &R);
    bam_reader_free_refs(&R);
    cornetto_pinned_free(pin[0]);
    cornetto_pinned_free(pin[1]);
    if (nomem)
        CLI_WARNING("%s: a record does not fit the window of %lld bytes with one more block (CORNETTO_BAM_WINDOW): reading the rest of the file on the host, one thread",
                    path, (long long)opt.window);
    return nomem;
}
