/* bgcomp.c — compressed depth files of `(no)boringbits` (mosdepth writes its per-base output as *.per-base.bed.gz only, which is BGZF).
 *   cli_depth_kind()     what a regular file is by its first bytes: BGZF, another gzip, or text; nothing else is ever looked at
 *   cli_zfile_open()     the file through zlib on this thread, as a FILE * (fopencookie): gzip files, every compressed file of the host path
 *                        (--accel=no) and BGZF files under CORNETTO_BGZF=0.  The readers behind it are the ones that read text
 *   cli_bgz_*()          a BGZF file for the device: compressed bytes go over the bus slab by slab, the host walks the chain, and the blocks are
 *                        handed to cornetto_bgin_feed_src() / cornetto_bgrun_feed_src(), which inflate them into their own text on the device
 * What is wrong with a compressed file is ONE error line that names the file (and, for BGZF, the block's index and its offset), exit status 1. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <zlib.h>

#include "cli.h"

#define BGZ_MEMBER_MAX 65536 /* BSIZE is 16 bits: a member has at most 65536 bytes */

int cli_bgzf_first_member(int fd)
{
    uint8_t *head = (uint8_t *)cli_xmalloc(BGZ_MEMBER_MAX);
    const int64_t have = cli_read_at(fd, (char *)head, BGZ_MEMBER_MAX, 0, NULL);
    cornetto_bgzf_block_t b;
    int64_t dst = 0, n = 0, resume = 0;
    int32_t broken = 0;
    const int ok = have > 0 && cornetto_bgzf_scan(head, have, 0, &dst, &b, 1, &n, &resume, &broken) == CORNETTO_OK && n == 1;
    free(head);
    return ok;
}

int cli_depth_kind(FILE *fp)
{
    struct stat st;
    const int fd = fileno(fp);
    if (fd < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return 0; /* FIFOs and the like: read as ever, never peeked into */
    if (cli_bgzf_first_member(fd)) return 1;
    unsigned char m[2] = {0, 0};
    return cli_read_at(fd, (char *)m, 2, 0, NULL) == 2 && m[0] == 0x1f && m[1] == 0x8b ? 2 : 0;
}

void cli_bgz_fail(const char *path, int what, long long index, long long offset)
{
    if (what == 0) {
        CLI_ERROR("%s: BGZF block %lld at offset %lld does not inflate to what its footer says", path, index, offset);
    } else if (what == 1) {
        CLI_ERROR("%s: BGZF block %lld at offset %lld: what follows the blocks in front of it is not a BGZF block", path, index, offset);
    } else {
        CLI_ERROR("%s: BGZF block %lld at offset %lld: the file ends inside the block", path, index, offset);
    }
    exit(EXIT_FAILURE);
}

/* the member that begins at buf (have bytes of the file at `off`, up to a whole member) -> 1 and the block (src counts from buf), 0 at the end of the file */
static int bgz_member(const char *path, const uint8_t *buf, int64_t have, int64_t off, long long index, cornetto_bgzf_block_t *b, int64_t *size)
{
    if (have <= 0) return 0;
    int64_t dst = 0, n = 0, resume = off;
    int32_t broken = 0;
    if (cornetto_bgzf_scan(buf, have, off, &dst, b, 1, &n, &resume, &broken) != CORNETTO_OK || broken) cli_bgz_fail(path, 1, index, (long long)off);
    if (n != 1) cli_bgz_fail(path, 2, index, (long long)off);
    b->src -= off;
    *size = resume - off;
    return 1;
}

/* ---------------------------------------------------------------- through zlib, as a FILE * */
typedef struct {
    char *path;
    FILE *fp;   /* the file as the caller opened it */
    gzFile gz;  /* kind 2 */
    /* kind 1 */
    int bgzf;
    int64_t off;
    long long index;
    uint8_t *in, *out;
    int64_t out_n, out_at;
} zfile_t;

static void zfile_next_block(zfile_t *z)
{
    int failed = 0;
    const int64_t have = cli_read_at(fileno(z->fp), (char *)z->in, BGZ_MEMBER_MAX, z->off, &failed);
    if (failed || have < 0) {
        CLI_ERROR("reading %s failed", z->path);
        exit(EXIT_FAILURE);
    }
    cornetto_bgzf_block_t b;
    int64_t size = 0;
    z->out_at = z->out_n = 0;
    if (!bgz_member(z->path, z->in, have, z->off, z->index, &b, &size)) {
        z->out_n = -1; /* the end of the file */
        return;
    }
    z_stream s;
    memset(&s, 0, sizeof(s));
    int ok = inflateInit2(&s, -15) == Z_OK;
    if (ok) {
        s.next_in = (Bytef *)(z->in + b.src);
        s.avail_in = (uInt)b.n_src;
        s.next_out = z->out;
        s.avail_out = (uInt)b.n_dst;
        const int zr = inflate(&s, Z_FINISH);
        /* (a stream that says more than ISIZE stops at Z_BUF_ERROR with the output full; one that says less ends early) */
        ok = zr == Z_STREAM_END && (int64_t)s.total_out == b.n_dst && s.avail_in == 0 &&
             (uint32_t)crc32(crc32(0L, Z_NULL, 0), z->out, (uInt)b.n_dst) == b.crc;
        inflateEnd(&s);
    }
    if (!ok) cli_bgz_fail(z->path, 0, z->index, (long long)z->off);
    z->out_n = b.n_dst;
    z->off += size;
    ++z->index;
}

static ssize_t zfile_read(void *cookie, char *buf, size_t size)
{
    zfile_t *z = (zfile_t *)cookie;
    if (!z->bgzf) {
        size_t got = 0;
        while (got < size) {
            const unsigned want = size - got > (1u << 30) ? (1u << 30) : (unsigned)(size - got);
            const int r = gzread(z->gz, buf + got, want);
            int zerr = Z_OK;
            const char *msg = gzerror(z->gz, &zerr);
            if (r < 0 || (zerr != Z_OK && zerr != Z_STREAM_END)) {
                CLI_ERROR("%s: not a gzip file to its end (%s)", z->path, zerr == Z_ERRNO ? "read error" : msg);
                exit(EXIT_FAILURE);
            }
            if (r == 0) break;
            got += (size_t)r;
        }
        return (ssize_t)got;
    }
    size_t got = 0;
    while (got < size && z->out_n >= 0) {
        if (z->out_at == z->out_n) {
            zfile_next_block(z);
            continue;
        }
        const size_t k = (size_t)(z->out_n - z->out_at) < size - got ? (size_t)(z->out_n - z->out_at) : size - got;
        memcpy(buf + got, z->out + z->out_at, k);
        z->out_at += (int64_t)k;
        got += k;
    }
    return (ssize_t)got;
}

static int zfile_close(void *cookie)
{
    zfile_t *z = (zfile_t *)cookie;
    if (z->gz) gzclose(z->gz);
    fclose(z->fp);
    free(z->in);
    free(z->out);
    free(z->path);
    free(z);
    return 0;
}

FILE *cli_zfile_open(const char *path, FILE *fp, int kind)
{
    zfile_t *z = (zfile_t *)cli_xmalloc(sizeof(*z));
    memset(z, 0, sizeof(*z));
    z->path = (char *)cli_xmalloc(strlen(path) + 1);
    strcpy(z->path, path);
    z->fp = fp;
    z->bgzf = kind == 1;
    if (z->bgzf) {
        z->in = (uint8_t *)cli_xmalloc(BGZ_MEMBER_MAX);
        z->out = (uint8_t *)cli_xmalloc(65536);
    } else if (!(z->gz = gzopen(path, "rb"))) {
        CLI_ERROR("Failed to open %s : No such file or directory.", path);
        exit(EXIT_FAILURE);
    }
    const cookie_io_functions_t io = {zfile_read, NULL, NULL, zfile_close};
    FILE *out = fopencookie(z, "r", io);
    if (!out) {
        CLI_ERROR("%s: cannot open a stream over the compressed file", path);
        exit(EXIT_FAILURE);
    }
    return out;
}

/* ---------------------------------------------------------------- a BGZF file for the device */
struct cli_bgz {
    char *path;
    int fd, n_rd;
    int64_t size, slab_cap;
    char *slab[2]; /* pinned: the blocks of slab[cur] are being fed while the reader fills the other */
    int cur;
    cornetto_text_t *comp; /* the current slab on the device */
    cornetto_bgzf_block_t *blocks;   /* the whole blocks of the current slab; src counts from the slab */
    int64_t *starts;                 /* where each of them begins in the file */
    int64_t n_blocks, at_block, cap_blocks;
    long long index0;                /* index in the file of blocks[0] */
    int64_t next_off;                /* file offset behind the last whole block of the current slab */
    int eof;                         /* the current slab's blocks are the file's last */
    /* the read ahead */
    pthread_t th;
    int th_started;
    int64_t rd_off, rd_want, rd_got;
};

static void *bgz_reader(void *p)
{
    cli_bgz_t *z = (cli_bgz_t *)p;
    z->rd_got = z->rd_want > 0 ? cli_pread_parallel(z->fd, z->slab[z->cur ^ 1], z->rd_want, z->rd_off, z->n_rd) : 0;
    return NULL;
}

static void bgz_post(cli_bgz_t *z, int64_t off)
{
    z->rd_off = off;
    z->rd_want = z->size - off < z->slab_cap ? z->size - off : z->slab_cap;
    z->th_started = pthread_create(&z->th, NULL, bgz_reader, z) == 0;
    if (!z->th_started) bgz_reader(z); /* no thread to be had: read here */
}

cli_bgz_t *cli_bgz_open(cornetto_accel_t *h, const char *path, int fd, int64_t slab_bytes, int n_rd)
{
    struct stat st;
    cli_bgz_t *z = (cli_bgz_t *)cli_xmalloc(sizeof(*z));
    memset(z, 0, sizeof(*z));
    z->path = (char *)cli_xmalloc(strlen(path) + 1);
    strcpy(z->path, path);
    z->fd = fd;
    z->n_rd = n_rd > 0 ? n_rd : 1;
    if (fstat(fd, &st) != 0) {
        CLI_ERROR("reading %s failed", path);
        exit(EXIT_FAILURE);
    }
    z->size = (int64_t)st.st_size;
    z->slab_cap = slab_bytes < z->size ? slab_bytes : z->size;                 /* (a small file: no more pinned memory than it has bytes) */
    if (z->slab_cap < BGZ_MEMBER_MAX) z->slab_cap = BGZ_MEMBER_MAX;            /* (a slab holds one whole member at least) */
    for (int i = 0; i < 2; ++i)
        if (!(z->slab[i] = (char *)cornetto_pinned_alloc((size_t)z->slab_cap))) {
            CLI_ERROR("%s", "cannot allocate pinned read buffers");
            exit(EXIT_FAILURE);
        }
    cli_accel_check(h, cornetto_text_open(h, z->slab_cap, &z->comp), "allocating the compressed text on the GPU");
    z->cap_blocks = z->slab_cap / 26 + 2; /* (no member is shorter than its 18 + 8 bytes of header and footer) */
    z->blocks = (cornetto_bgzf_block_t *)cli_xmalloc((size_t)z->cap_blocks * sizeof(*z->blocks));
    z->starts = (int64_t *)cli_xmalloc((size_t)z->cap_blocks * sizeof(*z->starts));
    z->cur = 1; /* (the first read goes into slab 0) */
    bgz_post(z, 0);
    return z;
}

/* the slab that has been read ahead becomes the current one: its chain is walked, it starts for the device, the next one starts to be read */
static void bgz_load(cornetto_accel_t *h, cli_bgz_t *z)
{
    if (z->th_started) pthread_join(z->th, NULL);
    z->th_started = 0;
    if (z->rd_got < 0) {
        CLI_ERROR("reading %s failed", z->path);
        exit(EXIT_FAILURE);
    }
    z->cur ^= 1;
    z->index0 += z->n_blocks;
    const int64_t off = z->rd_off, got = z->rd_got;
    int64_t dst = 0, nb = 0, resume = off;
    int32_t broken = 0;
    cli_accel_check(h, cornetto_bgzf_scan((const uint8_t *)z->slab[z->cur], got, off, &dst, z->blocks, z->cap_blocks, &nb, &resume, &broken), "BGZF chain");
    z->n_blocks = nb;
    z->at_block = 0;
    int64_t at = off;
    for (int64_t i = 0; i < nb; ++i) {
        z->starts[i] = at;
        at = z->blocks[i].src + z->blocks[i].n_src + 8; /* (the footer: CRC-32 and ISIZE) */
        z->blocks[i].src -= off;
    }
    z->next_off = resume;
    z->eof = resume >= z->size;
    /* the blocks in front of a place where the chain breaks, or where the file ends inside a block, are fed first: the next load says what is wrong */
    if (nb == 0) {
        if (broken) cli_bgz_fail(z->path, 1, z->index0, (long long)resume);
        if (!z->eof) cli_bgz_fail(z->path, 2, z->index0, (long long)resume);
        return;
    }
    cli_accel_check(h, cornetto_text_put(h, z->comp, z->slab[z->cur], got, 0, 0), "copying the compressed text to the GPU");
    if (!z->eof) bgz_post(z, resume);
}

int64_t cli_bgz_next(cornetto_accel_t *h, cli_bgz_t *z, int64_t want, cornetto_bgsrc_t *src, int *last)
{
    memset(src, 0, sizeof(*src));
    if (z->at_block == z->n_blocks && !z->eof) bgz_load(h, z);
    int64_t n = 0, bytes = 0;
    while (z->at_block + n < z->n_blocks && (n == 0 || bytes + z->blocks[z->at_block + n].n_dst <= want)) bytes += z->blocks[z->at_block + n++].n_dst;
    src->comp = z->comp;
    src->blocks = z->blocks + z->at_block;
    src->n_blocks = n;
    z->at_block += n;
    *last = z->eof && z->at_block == z->n_blocks;
    return bytes;
}

void cli_bgz_fail_block(const cli_bgz_t *z, long long index)
{
    const long long k = index - z->index0;
    cli_bgz_fail(z->path, 0, index, k >= 0 && k < z->n_blocks ? (long long)z->starts[k] : -1);
}

void cli_bgz_close(cornetto_accel_t *h, cli_bgz_t *z)
{
    if (!z) return;
    if (z->th_started) pthread_join(z->th, NULL); /* never leave a reader behind */
    cornetto_text_free(h, z->comp);
    cornetto_pinned_free(z->slab[0]);
    cornetto_pinned_free(z->slab[1]);
    free(z->blocks);
    free(z->starts);
    free(z->path);
    free(z);
}
