/* bam.c — `(no)boringbits --bam FILE`: both coverage tracks from the BAM on the device (an extension; include/cornetto_accel.h states the
 * rules).  The compressed file is read a chunk at a time into ONE pinned slab (no ring, no reader thread yet: read, upload and kernels follow
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

int cli_bam_ingest(cornetto_accel_t *h, const char *path, int min_mapq, cornetto_cov_t **cov, int32_t *n_ctg, char ***names, int64_t *n_clamped)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        CLI_ERROR("Failed to open %s : No such file or directory.", path);
        exit(EXIT_FAILURE);
    }
    cornetto_bamdepth_opt_t opt;
    cornetto_bamdepth_defaults(&opt);
    opt.min_mapq = min_mapq;
    if (getenv("CORNETTO_BAM_WINDOW")) {
        char *end = NULL;
        const long long w = strtoll(getenv("CORNETTO_BAM_WINDOW"), &end, 10);
        if (end == getenv("CORNETTO_BAM_WINDOW") || *end || w < 1 || w > 0xF0000000ll) {
            CLI_ERROR("CORNETTO_BAM_WINDOW wants a number of bytes from 1 to %lld. Found %s", 0xF0000000ll, getenv("CORNETTO_BAM_WINDOW"));
            exit(EXIT_FAILURE);
        }
        opt.window = w;
    }
    int64_t chunk = opt.window > (1ll << 20) ? opt.window : 1ll << 20;      /* compressed bytes per feed: a feed fills a window whatever the ratio */
    if (chunk > (1ll << 30)) chunk = 1ll << 30;
    if (fseek(fp, 0, SEEK_END) == 0) {      /* (a small file: a small slab) */
        const int64_t size = (int64_t)ftell(fp);
        if (size >= 0 && size + 65536 < chunk) chunk = size + 65536;
        rewind(fp);
    }
    uint8_t *slab = (uint8_t *)cornetto_pinned_alloc((size_t)chunk);
    const int64_t cap_blocks = chunk / 26 + 1;
    cornetto_bgzf_block_t *blocks = (cornetto_bgzf_block_t *)cli_xmalloc((size_t)cap_blocks * sizeof(cornetto_bgzf_block_t));
    if (!slab) {
        CLI_ERROR("%s", "cannot allocate the pinned read buffer");
        exit(EXIT_FAILURE);
    }
    cornetto_text_t *comp = NULL;
    cli_accel_check(h, cornetto_text_open(h, chunk, &comp), "BAM ingest");
    cornetto_bamdepth_t *b = NULL;
    uint8_t *hdr = NULL;
    int64_t n_hdr = 0, cap_hdr = 0, hdr_blocks = 0, file_off = 0, pend = 0, dst = 0;
    int32_t n_ref = 0, *ref_len = NULL;
    char **ref_name = NULL;
    int nomem = 0;
    for (int eof = 0; !eof;) {
        const size_t want = (size_t)(chunk - pend), got = fread(slab + pend, 1, want, fp);
        eof = got < want;
        const int64_t n = pend + (int64_t)got;
        int64_t nb = 0, resume = file_off;
        int32_t broken = 0;
        cli_accel_check(h, cornetto_bgzf_scan(slab, n, file_off, &dst, blocks, cap_blocks, &nb, &resume, &broken), "BGZF chain");
        const int64_t used = resume - file_off;
        if (broken || (eof && used < n) || (!eof && used == 0)) cli_bam_fail(path, b ? 6 : 7, 0, 0, 0);
        for (int64_t i = 0; i < nb; ++i) blocks[i].src -= file_off;
        int64_t skip = 0;
        if (!b) {       /* the header: as many leading blocks as it takes */
            int rc = 1;
            while (rc == 1 && hdr_blocks < nb) {
                if (bam_inflate_block(slab, &blocks[hdr_blocks++], &hdr, &n_hdr, &cap_hdr) != 0) cli_bam_fail(path, 6, 0, 0, 0);
                int64_t hb = 0;
                rc = cornetto_bam_header(hdr, n_hdr, &n_ref, &ref_name, &ref_len, &hb);
                skip = hb;
            }
            if (rc == 1 && eof) cli_bam_fail(path, 2, -1, 0, -1);
            if (rc == 1) {
                CLI_ERROR("%s: a BAM header of more than %lld compressed bytes", path, (long long)chunk);
                exit(EXIT_FAILURE);
            }
            if (rc != CORNETTO_OK) cli_bam_fail(path, 7, -1, 0, 0);
            rc = cornetto_bamdepth_open(h, &opt, ref_len, n_ref, &b);
            if (rc == CORNETTO_E_NOMEM) {
                nomem = 2;
                break;
            }
            cli_accel_check(h, rc, "BAM ingest");
        }
        if (used > 0) cli_accel_check(h, cornetto_text_put(h, comp, (const char *)slab, used, 0, 0), "BAM upload");
        const int rc = cornetto_bamdepth_feed(h, b, comp, blocks, nb, skip);
        if (rc == CORNETTO_E_NOMEM) {
            nomem = 1;
            break;
        }
        if (rc != CORNETTO_OK) bam_device_fail(h, path, b, rc);
        pend = n - used;
        if (pend > 0) memmove(slab, slab + used, (size_t)pend);
        file_off = resume;
    }
    fclose(fp);
    free(hdr);
    free(blocks);
    int rc = CORNETTO_OK;
    cornetto_cov_t *c = NULL;
    if (!nomem) {
        if (!b) cli_bam_fail(path, 2, -1, 0, -1);      /* (an empty file) */
        rc = cornetto_bamdepth_finish(h, b, &c, NULL, NULL, n_clamped);
        if (rc == CORNETTO_E_NOMEM) nomem = 2;
        else if (rc != CORNETTO_OK) bam_device_fail(h, path, b, rc);
    }
    cornetto_bamdepth_close(h, b);
    cornetto_text_free(h, comp);
    cornetto_pinned_free(slab);
    if (nomem) {
        if (nomem == 1)
            CLI_WARNING("%s: a record does not fit the window of %lld bytes with one more block (CORNETTO_BAM_WINDOW): reading the file on the host, one thread",
                        path, (long long)opt.window);
        else
            CLI_WARNING("%s: the device has no room for the depth arrays of the %d contigs of the header: reading the file on the host, one thread", path, n_ref);
        for (int32_t i = 0; i < n_ref; ++i) free(ref_name[i]);
        free(ref_name);
        free(ref_len);
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
