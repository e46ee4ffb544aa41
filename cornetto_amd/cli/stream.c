/* stream.c — the FASTA/FASTQ record streamer of the device path: stream_records() (telofind, sdust, fixasm) and stream_names() (nx, report,
 * telocontigs, asmstats).  The records are framed on the device wherever the text is plain (cornetto_fasta_split_text, cornetto_fasta_split,
 * cornetto_fastq_split) and handed to the caller's scan in input order.  Anything else — wrapped FASTQ, stray lines, a FASTQ record inside a FASTA
 * file, the reference's error cases — is read by the sequential reader (cli/fastx.c) from the first byte the device was not sure about: the
 * output is kseq's either way (src/kseq.h:184-224 as called at src/find_telomere.c:101, src/sdust/sdust.c:196).
 * stream_run() looks at the input once and picks one of four sources:
 *   stream_whole_fasta()  an uncompressed regular FASTA file as ONE text on the device;
 *   stream_bgzf_fasta()   a BGZF-compressed (bgzip) regular FASTA file: uploaded as it is, inflated on the device into ONE text;
 *   stream_pieces()       gzip, stdin, FASTQ, CORNETTO_CLI_WHOLE=0 or CORNETTO_FASTQ_PIECE (bytes per piece): pinned pieces, framed one by one;
 *   stream_sequential()   what those two leave, or everything (CORNETTO_FASTQ_SPLIT=host, text that begins with neither '>' nor '@'). */
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "cli.h"

#define WHOLE_SLOTS 16

typedef struct {
    const char *path;
    scan_fn scan;
    void *arg;
    int names_only;          /* stream_names(): the framing gets seqs == NULL, the scan a == NULL, the sequential reader uploads nothing */
    int release;             /* stream_records_on(): what the call allocated is released before it returns, as for stream_names() */
    int warm;                /* CORNETTO_WARM_* for a large assembly, or 0 */
    cornetto_accel_t *h;     /* NULL until the first device call needs it (cli_accel_open_end) */
    int trace;               /* CORNETTO_CLI_TRACE */
    double t_begin;
    gzFile fp;
    int64_t size;            /* of an uncompressed regular file, else -1 */
    int raw_fd;              /* such a file opened for pread(): its bytes are the stream's bytes; else -1 */
    int64_t raw_off;         /* the pieces' read position in it */
    /* what this call allocated: stream_release() */
    cornetto_text_t *text;
    char *pinned[WHOLE_SLOTS];
    int n_pinned;
} stream_t;

#define TRACE(what)                                                                                               \
    do {                                                                                                          \
        if (s->trace) fprintf(stderr, "[cli trace] %-28s %8.1f ms\n", (what), (cli_realtime() - s->t_begin) * 1e3); \
    } while (0)

/* one thread copies from the page cache at 5-8 GB/s: the largest share of the wall time of a 3 GB assembly */
static int read_threads(void)
{
    const char *e = getenv("CORNETTO_READ_THREADS");
    const int v = e ? atoi(e) : 8;
    return v < 1 ? 1 : v;
}

/* ---------------------------------------------------------------- the sequential reader */
/* a batch of it: upload, then the same scan */
static void scan_batch(cli_batch_t *b, void *arg)
{
    stream_t *s = (stream_t *)arg;
    if (!s->h) s->h = cli_accel_open_end();
    cornetto_asm_t *a = NULL;
    cli_accel_check(s->h, cornetto_asm_upload(s->h, (const uint8_t *const *)b->seqs, b->lens, b->n, &a), "copying sequences to the GPU");
    cli_recname_t *r = (cli_recname_t *)cli_xmalloc(((size_t)b->n + 1) * sizeof(*r));
    for (int32_t i = 0; i < b->n; ++i) {
        r[i].name = b->names[i];
        r[i].name_len = (int32_t)strlen(b->names[i]);
        r[i].len = b->lens[i];
    }
    s->scan(s->h, r, b->n, a, s->arg);
    free(r);
    cornetto_asm_free(s->h, a);
}

/* `n` bytes at `prefix`, then the rest of s->fp (closed here).  names_only: every record's name and length handed over one at a time */
static void stream_sequential(stream_t *s, const char *prefix, size_t n)
{
    cli_fastx_t *fx = cli_fastx_open_prefixed(s->fp, prefix, n);
    if (s->names_only) {
        cli_rec_t *rec;
        while ((rec = cli_fastx_next(fx)) != NULL) {
            const cli_recname_t r = {rec->name.s, (int32_t)rec->name.l, (int64_t)rec->seq.l};
            s->scan(s->h, &r, 1, NULL, s->arg);
        }
        cli_fastx_close(fx);
        return;
    }
    if (!s->h) cli_accel_open_begin();     /* HIP initialises while the records are read */
    cli_fastx_batches(fx, scan_batch, s);
    if (!s->h) cli_accel_open_cancel();    /* (an input without records) */
}

/* ---------------------------------------------------------------- the piece loop */
static int64_t piece_bytes(int fasta, int64_t file_size)
{
    const char *e = getenv("CORNETTO_FASTQ_PIECE");
    int64_t v = e ? atoll(e) : 0;
    if (v < 64) {
        v = 256LL << 20;
        if (fasta) { /* a record must fit into a piece: the whole file at once when its size is known; else grown on demand */
            v = file_size >= 0 ? file_size + 16 : 64LL << 20;
            if (v > (256LL << 20)) v = 256LL << 20; /* (pinning and unpinning 1 GiB cost 0.27 s of a 0.9 s run; a longer record grows the piece) */
        }
    }
    if (v > 0xF0000000LL) v = 0xF0000000LL;
    return v;
}

/* up to `want` bytes of the input behind the ones read so far -> how many; fewer than `want`: the input ends there */
static int64_t piece_fill(stream_t *s, char *dst, int64_t want)
{
    int64_t got = 0;
    if (s->raw_fd >= 0) {
        got = cli_pread_parallel(s->raw_fd, dst, want, s->raw_off, read_threads());
        if (got > 0) s->raw_off += got;
    }
    while (s->raw_fd < 0 && got >= 0 && got < want) {
        const int64_t ask = want - got > (1 << 30) ? (1 << 30) : want - got;
        const int r = gzread(s->fp, dst + got, (unsigned)ask);
        got = r < 0 ? -1 : got + r;
        if (r < ask) break;
    }
    if (got < 0) {
        CLI_ERROR("reading %s failed", s->path);
        if (!s->h) cli_accel_open_cancel();    /* (exit() beside a device that is still being opened on the helper thread ends with SIGSEGV) */
        exit(EXIT_FAILURE);
    }
    return got;
}

/* the plain records at the head of buf[0 .. have): names point into buf.  *a: their sequences on the device (not for names_only) */
static cli_recname_t *piece_frame(stream_t *s, int fasta, const char *buf, int64_t have, int eof, int64_t *n, int64_t *used, int32_t *plain, cornetto_asm_t **a)
{
    cornetto_farec_t *fa = NULL;
    cornetto_fqrec_t *fq = NULL;
    cornetto_asm_t **seqs = s->names_only ? NULL : a;
    if (fasta) cli_accel_check(s->h, cornetto_fasta_split(s->h, buf, have, eof, &fa, n, used, plain, seqs), "framing the FASTA records");
    else cli_accel_check(s->h, cornetto_fastq_split(s->h, buf, have, eof, 0, &fq, n, used, plain, seqs), "framing the FASTQ records");
    cli_recname_t *r = (cli_recname_t *)cli_xmalloc(((size_t)*n + 1) * sizeof(*r));
    for (int64_t i = 0; i < *n; ++i) {
        r[i].name = buf + (fasta ? fa[i].head : fq[i].head) + 1;
        r[i].name_len = fasta ? fa[i].name_len : fq[i].name_len;
        r[i].len = fasta ? fa[i].len : fq[i].len;
    }
    cornetto_free(fa);
    cornetto_free(fq);
    return r;
}

/* The input goes to the device in pinned pieces as it is: fill, frame, scan, carry the unconsumed tail to the front, and grow the piece when one
 * record does not fit.  `first` is the byte already read.  A piece size given by hand is kept (tests: records that do not fit go to the sequential
 * reader) unless CORNETTO_FASTQ_GROW=1 asks for the growth path as well.
 * -> 1: *rest[0 .. *n_rest) and what follows in s->fp are for the sequential reader (not plain there, or a record no piece can hold) */
static int stream_pieces(stream_t *s, char first, const char **rest, size_t *n_rest)
{
    const int fasta = first == '>';
    int64_t cap = piece_bytes(fasta, s->size);
    const char *grow = getenv("CORNETTO_FASTQ_GROW");
    const int64_t cap_max = getenv("CORNETTO_FASTQ_PIECE") && !(grow && atoi(grow)) ? cap : 0xF0000000LL;
    char *buf = (char *)cornetto_pinned_alloc((size_t)cap);
    if (!buf) {
        s->h = cli_accel_open_end(); /* no usable device: its message and exit(EXIT_FAILURE) */
        CLI_ERROR("could not allocate a %lld-byte pinned read buffer", (long long)cap);
        exit(EXIT_FAILURE);
    }
    buf[0] = first;
    TRACE("pinned piece allocated");
    int64_t have = 1, start = 0; /* unread bytes: buf[start .. have) */
    int eof = 0;
    s->raw_off = 1;
    for (;;) {
        if (start) {
            memmove(buf, buf + start, (size_t)(have - start));
            have -= start;
            start = 0;
        }
        if (have < cap && !eof) {
            const int64_t want = cap - have, got = piece_fill(s, buf + have, want);
            have += got;
            if (got < want) eof = 1;
        }
        if (have == 0) break;
        TRACE("piece read");
        if (!s->h) s->h = cli_accel_open_end();
        TRACE("device open");
        cornetto_asm_t *a = NULL;
        int64_t n = 0, used = 0;
        int32_t plain = 1;
        cli_recname_t *r = piece_frame(s, fasta, buf, have, eof, &n, &used, &plain, &a);
        TRACE("records framed");
        if (n) s->scan(s->h, r, n, a, s->arg);
        TRACE("scanned and printed");
        free(r);
        cornetto_asm_free(s->h, a);
        start = used;
        if (!plain || eof) break;              /* not plain from buf + start on / the input is finished */
        if (used == 0 && have == cap) {        /* one record larger than the piece: a larger one, as long as the index allows */
            if (cap >= cap_max) break;
            const int64_t bigger = cap * 2 > cap_max ? cap_max : cap * 2;
            char *nb = (char *)cornetto_pinned_alloc((size_t)bigger);
            if (!nb) break;
            memcpy(nb, buf, (size_t)have);
            cornetto_pinned_free(buf);
            buf = nb;
            cap = bigger;
        }
    }
    s->pinned[s->n_pinned++] = buf;
    if (s->raw_fd >= 0) { /* the sequential reader goes on in the gz stream where the raw reads stopped */
        close(s->raw_fd);
        gzseek(s->fp, (z_off_t)s->raw_off, SEEK_SET);
    }
    *rest = buf + start;
    *n_rest = (size_t)(have - start);
    return start < have || !eof;
}

/* ---------------------------------------------------------------- an uncompressed FASTA FILE as ONE text on the device
 * The piece loop above pins buffers that must each hold whole records (256 MiB and more for an assembly), reads every contig that
 * straddles a piece border twice, and frames, uploads and scans a dozen pieces one after the other, each a cold first pass over a new
 * resident object: 0.45-0.63 s for the 3.16 GB assembly of which 0.15 s were the scans' pipeline.  Here the file goes through a small ring
 * of pinned slabs (reader threads fill them from the page cache, four copy queues empty them: cornetto_text_put) into one device buffer, and
 * the whole text is framed and scanned ONCE (cornetto_fasta_split_text).  Record names are read back from the file by offset.  Texts are
 * limited to 2^32-256 bytes: a longer file takes several rounds, each ending at its last complete record. */
typedef struct {
    int fd, n_slots, failed, pin_failed;
    int64_t off0, total, slab, n_slab;
    char *ring[WHOLE_SLOTS];
    int64_t filled[WHOLE_SLOTS];  /* slab index + 1 the slot holds (0: none) */
    int64_t allowed[WHOLE_SLOTS]; /* the slab index the slot may be filled with */
    int64_t got[WHOLE_SLOTS];     /* bytes of it */
    int64_t next;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    pthread_t pin_th;
    int pin_started;
} whole_ring_t;

static void *whole_reader(void *p)
{
    whole_ring_t *w = (whole_ring_t *)p;
    for (;;) {
        pthread_mutex_lock(&w->mu);
        const int64_t i = w->next++;
        if (i >= w->n_slab || w->failed) {
            pthread_mutex_unlock(&w->mu);
            return NULL;
        }
        const int sl = (int)(i % w->n_slots);
        while ((w->allowed[sl] != i || !w->ring[sl]) && !w->failed && !w->pin_failed) pthread_cond_wait(&w->cv, &w->mu);
        const int stop = w->failed || w->pin_failed;
        pthread_mutex_unlock(&w->mu);
        if (stop) return NULL;
        const int64_t at = i * w->slab, want = w->total - at < w->slab ? w->total - at : w->slab;
        const int64_t have = cli_read_at(w->fd, w->ring[sl], want, w->off0 + at, NULL);
        pthread_mutex_lock(&w->mu);
        if (have < want) w->failed = 1;          /* (a file that shrank under us, an I/O error) */
        w->got[sl] = have;
        w->filled[sl] = i + 1;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
    }
}

/* the slabs are page-locked one after the other (~5-20 GB/s: 128 MB take 10-25 ms) by a thread of their own, while the first ones are already
 * being filled and copied */
static void *whole_pinner(void *p)
{
    whole_ring_t *w = (whole_ring_t *)p;
    for (int sl = 0; sl < w->n_slots; ++sl) {
        char *m = (char *)cornetto_pinned_alloc((size_t)w->slab);
        pthread_mutex_lock(&w->mu);
        if (!m) w->pin_failed = 1;
        w->ring[sl] = m;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        if (!m) return NULL;
    }
    return NULL;
}

/* the ring for a text of `cap` bytes read from fd -> the number of reader threads.  `w` must stay where it is until whole_ring_close() */
static int whole_ring_open(whole_ring_t *w, int fd, int64_t cap)
{
    memset(w, 0, sizeof(*w));
    pthread_mutex_init(&w->mu, NULL);
    pthread_cond_init(&w->cv, NULL);
    w->fd = fd;
    /* sixteen slabs of 8 MiB: a reader thread per slab in flight copies from the page cache at 4-6 GB/s, the copy queues take ~45 GB/s */
    w->slab = 8LL << 20;
    if (cap < w->slab * WHOLE_SLOTS) w->slab = ((cap + WHOLE_SLOTS - 1) / WHOLE_SLOTS + 65535) & ~65535LL;   /* (a small file: a small ring) */
    w->n_slots = (int)((cap + w->slab - 1) / w->slab);
    if (w->n_slots > WHOLE_SLOTS) w->n_slots = WHOLE_SLOTS;
    if (w->n_slots < 1) w->n_slots = 1;
    w->pin_started = pthread_create(&w->pin_th, NULL, whole_pinner, w) == 0;
    if (!w->pin_started) whole_pinner(w);
    int n_thr = getenv("CORNETTO_READ_THREADS") ? read_threads() : 16;
    if (n_thr > w->n_slots) n_thr = w->n_slots;
    return n_thr;
}

/* the slabs go to the stream (stream_release()) */
static void whole_ring_close(stream_t *s, whole_ring_t *w)
{
    if (w->pin_started) pthread_join(w->pin_th, NULL);   /* (it uses `w`) */
    for (int sl = 0; sl < w->n_slots; ++sl) s->pinned[s->n_pinned++] = w->ring[sl];
    pthread_mutex_destroy(&w->mu);
    pthread_cond_destroy(&w->cv);
}

/* bytes [off, off + n) of the file through the ring into the device text */
static void whole_put(stream_t *s, whole_ring_t *w, int n_thr, int64_t off, int64_t n)
{
    w->off0 = off;
    w->total = n;
    w->n_slab = (n + w->slab - 1) / w->slab;
    w->next = 0;
    w->failed = 0;
    for (int sl = 0; sl < w->n_slots; ++sl) { w->filled[sl] = 0; w->allowed[sl] = sl; }
    pthread_t th[64];
    int n_started = 0;
    for (int k = 0; k < n_thr && k < 64; ++k)
        if (pthread_create(&th[n_started], NULL, whole_reader, w) == 0) ++n_started;
    if (n_started == 0) { CLI_ERROR("could not start a reader thread"); exit(EXIT_FAILURE); }
    for (int64_t i = 0; i < w->n_slab; ++i) {
        const int sl = (int)(i % w->n_slots);
        pthread_mutex_lock(&w->mu);
        while (w->filled[sl] != i + 1 && !w->failed && !w->pin_failed) pthread_cond_wait(&w->cv, &w->mu);
        const int64_t got = w->got[sl];
        const int failed = w->pin_failed ? 2 : w->failed;
        pthread_mutex_unlock(&w->mu);
        if (failed == 2) { CLI_ERROR("could not allocate a %lld-byte pinned slab", (long long)w->slab); exit(EXIT_FAILURE); }
        if (failed) { CLI_ERROR("reading %s failed", s->path); exit(EXIT_FAILURE); }
        /* four copy queues: slab i goes out on queue i & 3 once the copy that used that queue last (slab i - 4) has left its slab, which then
         * goes back to the readers: up to four copies in flight */
        if (i >= 4) {
            cli_accel_check(s->h, cornetto_text_wait(s->h, s->text, (int)(i & 3)), "copying the text to the GPU");
            const int sp = (int)((i - 4) % w->n_slots);
            pthread_mutex_lock(&w->mu);
            w->allowed[sp] = i - 4 + w->n_slots;
            pthread_cond_broadcast(&w->cv);
            pthread_mutex_unlock(&w->mu);
        }
        cli_accel_check(s->h, cornetto_text_put(s->h, s->text, w->ring[sl], got, i * w->slab, (int)(i & 3)), "copying the text to the GPU");
    }
    for (int k = 0; k < n_started; ++k) pthread_join(th[k], NULL);
}

/* the names of the text's records: from the file, by offset (the slabs are gone).  -> r[0 .. nrec), its names in *names_out */
static cli_recname_t *whole_names(stream_t *s, int64_t off, const cornetto_farec_t *recs, int64_t nrec, char **names_out)
{
    cli_recname_t *r = (cli_recname_t *)cli_xmalloc(((size_t)nrec + 1) * sizeof(*r));
    int64_t name_bytes = 0;
    for (int64_t i = 0; i < nrec; ++i) name_bytes += recs[i].name_len + 1;
    char *names = (char *)cli_xmalloc((size_t)name_bytes + 1), *q = names;
    for (int64_t i = 0; i < nrec; ++i) {
        int64_t have = 0;
        while (have < recs[i].name_len) {
            const ssize_t g = pread(s->raw_fd, q + have, (size_t)(recs[i].name_len - have), (off_t)(off + recs[i].head + 1 + have));
            if (g < 0 && errno == EINTR) continue;
            if (g <= 0) { CLI_ERROR("reading %s failed", s->path); exit(EXIT_FAILURE); }
            have += g;
        }
        r[i].name = q;
        r[i].name_len = recs[i].name_len;
        r[i].len = recs[i].len;
        q += recs[i].name_len + 1;
    }
    *names_out = names;
    return r;
}

/* -> the file offset up to which the records were handled: s->size, or less when the sequential reader must go on from there (text that is not
 * plain FASTA, one record longer than a text) */
static int64_t stream_whole_fasta(stream_t *s)
{
    const int64_t LIMIT = 0xFFFFFF00LL - 4096, size = s->size;
    if (!s->h) s->h = cli_accel_open_end();
    TRACE("device open");
    const int64_t cap = size < LIMIT ? size : LIMIT;
    cli_accel_check(s->h, cornetto_text_open(s->h, cap, &s->text), "allocating the text on the GPU");
    TRACE("device text allocated");
    whole_ring_t w;
    const int n_thr = whole_ring_open(&w, s->raw_fd, cap);
    int64_t off = 0;
    int plain_all = 1;
    while (off < size && plain_all) {
        const int64_t n = size - off < cap ? size - off : cap;
        const int final = off + n == size;
        whole_put(s, &w, n_thr, off, n);
        TRACE("text on the device");
        cornetto_farec_t *recs = NULL;
        cornetto_asm_t *a = NULL;
        int64_t nrec = 0, used = 0;
        int32_t plain = 1;
        cli_accel_check(s->h, cornetto_fasta_split_text(s->h, s->text, n, final, &recs, &nrec, &used, &plain, s->names_only ? NULL : &a), "framing the FASTA records");
        TRACE("records framed");
        if (nrec) {
            char *names = NULL;
            cli_recname_t *r = whole_names(s, off, recs, nrec, &names);
            s->scan(s->h, r, nrec, a, s->arg);
            TRACE("scanned and printed");
            free(names);
            free(r);
        }
        cornetto_free(recs);
        cornetto_asm_free(s->h, a);
        off += used;
        if (!plain) plain_all = 0;                 /* what follows at `off` is for the sequential reader */
        else if (used == 0 && !final) plain_all = 0; /* one record longer than a text (2^32 bytes): the sequential reader reports it as the reference's reader would */
        else if (final) off = size;
    }
    whole_ring_close(s, &w);
    return off;
}

/* ---------------------------------------------------------------- a BGZF-compressed FASTA FILE, inflated on the device
 * gzread() inflates on one host thread (the reference's reader: src/find_telomere.c:96, src/kseq.h:234) while the device waits.  bgzip output is
 * a chain of independent gzip members of at most 64 KiB with their sizes in the headers: the file goes to the device as it is, through the same
 * slab ring; a host thread walks the chain beside the upload (cornetto_bgzf_scan over the mapped file: no system call per block); the device
 * inflates a block per wave and checks every CRC-32 (cornetto_text_inflate); the text is framed and scanned ONCE as an uncompressed file's is,
 * and the record names come back packed (cornetto_text_gather).  Nothing is printed before the whole text has inflated cleanly: whatever is
 * not a sound BGZF chain of a text that fits goes through the piece loop from its first byte, as it always did. */
typedef struct {
    int fd;
    int64_t size;
    cornetto_bgzf_block_t *blocks;
    int64_t n, total;
    const char *why;          /* NULL: the chain ends with the file */
} bgzf_walk_t;

static void *bgzf_walker(void *p)
{
    bgzf_walk_t *k = (bgzf_walk_t *)p;
    void *m = mmap(NULL, (size_t)k->size, PROT_READ, MAP_PRIVATE, k->fd, 0);
    if (m == MAP_FAILED) { k->why = "the file cannot be mapped"; return NULL; }
    int64_t cap = k->size / 16384 + 64, at = 0;
    k->blocks = (cornetto_bgzf_block_t *)cli_xmalloc((size_t)cap * sizeof(*k->blocks));
    while (at < k->size) {
        if (k->n == cap) {
            cap *= 2;
            cornetto_bgzf_block_t *nb = (cornetto_bgzf_block_t *)cli_xmalloc((size_t)cap * sizeof(*nb));
            memcpy(nb, k->blocks, (size_t)k->n * sizeof(*nb));
            free(k->blocks);
            k->blocks = nb;
        }
        int64_t got = 0, resume = at;
        int32_t broken = 0;
        if (cornetto_bgzf_scan((const uint8_t *)m + at, k->size - at, at, &k->total, k->blocks + k->n, cap - k->n, &got, &resume, &broken) != CORNETTO_OK) broken = 1;
        k->n += got;
        at = resume;
        if (broken) { k->why = "the chain breaks"; break; }
        if (got == 0) { k->why = "bytes behind the last block"; break; }
    }
    munmap(m, (size_t)k->size);
    return NULL;
}

static void bgzf_fallback(stream_t *s, const char *why)
{
    if (s->trace) fprintf(stderr, "[cli trace] bgzf: fallback (%s)\n", why);
}

/* the names of the text's records, packed on the device and copied once -> r[0 .. nrec), its names in *names_out */
static cli_recname_t *bgzf_names(stream_t *s, const cornetto_farec_t *recs, int64_t nrec, char **names_out)
{
    cli_recname_t *r = (cli_recname_t *)cli_xmalloc(((size_t)nrec + 1) * sizeof(*r));
    int64_t *at = (int64_t *)cli_xmalloc(((size_t)nrec + 1) * sizeof(*at)), name_bytes = 0;
    int32_t *len = (int32_t *)cli_xmalloc(((size_t)nrec + 1) * sizeof(*len));
    for (int64_t i = 0; i < nrec; ++i) {
        at[i] = recs[i].head + 1;
        len[i] = recs[i].name_len;
        name_bytes += recs[i].name_len;
    }
    char *names = (char *)cli_xmalloc((size_t)name_bytes + 1), *q = names;
    cli_accel_check(s->h, cornetto_text_gather(s->h, s->text, at, len, nrec, names), "fetching the record names");
    for (int64_t i = 0; i < nrec; ++i) {
        r[i].name = q;
        r[i].name_len = recs[i].name_len;
        r[i].len = recs[i].len;
        q += recs[i].name_len;
    }
    free(at);
    free(len);
    *names_out = names;
    return r;
}

/* -> 0: not taken, nothing has been printed and s->fp is where it was: the piece loop goes on from the first byte.  1: the records up to the
 * offset *resume of the INFLATED text were handled; *total is that text's size (less: the sequential reader goes on at *resume) */
static int stream_bgzf_fasta(stream_t *s, int64_t csize, int64_t *resume, int64_t *total)
{
    const int64_t LIMIT = 0xFFFFFF00LL - 4096;
    const int n_pinned0 = s->n_pinned;
    bgzf_walk_t k;
    memset(&k, 0, sizeof(k));
    k.fd = open(s->path, O_RDONLY);
    if (k.fd < 0) { bgzf_fallback(s, "the file cannot be opened again"); return 0; }
    k.size = csize;
    const char *why = NULL;
    cornetto_text_t *comp = NULL;
    if (csize > LIMIT) why = "the file is larger than a device text";
    pthread_t walk_th;
    const int walk_started = !why && pthread_create(&walk_th, NULL, bgzf_walker, &k) == 0;
    if (!why) {
        if (!s->h) s->h = cli_accel_open_end();
        TRACE("device open");
        const int rc = cornetto_text_open(s->h, csize, &comp);
        if (rc == CORNETTO_E_NOMEM) why = "no device memory for the compressed text";
        else cli_accel_check(s->h, rc, "allocating the text on the GPU");
    }
    if (!why) {
        whole_ring_t w;
        const int n_thr = whole_ring_open(&w, k.fd, csize);
        s->text = comp;
        whole_put(s, &w, n_thr, 0, csize);
        s->text = NULL;
        whole_ring_close(s, &w);
        TRACE("compressed text on the device");
    }
    if (walk_started) pthread_join(walk_th, NULL);
    else if (!why) bgzf_walker(&k);
    close(k.fd);
    if (!why) {
        TRACE("block chain walked");
        why = k.why;
    }
    if (!why && k.total > LIMIT) why = "the text is larger than a device text";
    if (!why) {
        const int rc = cornetto_text_open(s->h, k.total > 0 ? k.total : 1, &s->text);
        if (rc == CORNETTO_E_NOMEM) why = "no device memory for the text";
        else cli_accel_check(s->h, rc, "allocating the text on the GPU");
    }
    if (!why) {
        int64_t first_bad = -1;
        const int rc = cornetto_text_inflate(s->h, comp, s->text, k.blocks, k.n, &first_bad);
        if (rc == CORNETTO_E_FORMAT && first_bad >= 0) why = "a block is not what its footer says";
        else if (rc == CORNETTO_E_NOMEM) why = "no device memory for the block table";
        else cli_accel_check(s->h, rc, "inflating the text on the GPU");
    }
    if (comp) cornetto_text_free(s->h, comp);
    free(k.blocks);
    if (why) {
        if (s->text) cornetto_text_free(s->h, s->text);
        s->text = NULL;
        while (s->n_pinned > n_pinned0) cornetto_pinned_free(s->pinned[--s->n_pinned]);   /* the ring's slabs: the piece loop pins its own */
        bgzf_fallback(s, why);
        return 0;
    }
    TRACE("text inflated on the device");
    cornetto_farec_t *recs = NULL;
    cornetto_asm_t *a = NULL;
    int64_t nrec = 0, used = 0;
    int32_t plain = 1;
    cli_accel_check(s->h, cornetto_fasta_split_text(s->h, s->text, k.total, 1, &recs, &nrec, &used, &plain, s->names_only ? NULL : &a), "framing the FASTA records");
    TRACE("records framed");
    if (nrec) {
        char *names = NULL;
        cli_recname_t *r = bgzf_names(s, recs, nrec, &names);
        s->scan(s->h, r, nrec, a, s->arg);
        TRACE("scanned and printed");
        free(names);
        free(r);
    }
    cornetto_free(recs);
    cornetto_asm_free(s->h, a);
    *resume = plain ? k.total : used;     /* not plain: what follows at `used` is for the sequential reader */
    *total = k.total;
    return 1;
}

/* ---------------------------------------------------------------- one call */
/* stream_names() is called once per file, so nothing may pile up: the text and the pinned slabs and pieces are freed, and s->h goes back to the
 * caller.  stream_records() leaves them and the device handle to the end of the process (main.c leaves with _exit right after the sub-command):
 * unpinning a 1 GB piece and closing the handle take about 0.1 s. */
static void stream_release(stream_t *s)
{
    if (!s->names_only && !s->release) return;
    for (int i = 0; i < s->n_pinned; ++i) cornetto_pinned_free(s->pinned[i]);
    if (s->text) cornetto_text_free(s->h, s->text);
}

static void stream_run(stream_t *s, int must_open)
{
    s->trace = getenv("CORNETTO_CLI_TRACE") != NULL;
    s->t_begin = cli_realtime();
    s->fp = (gzFile)cli_gz_open(s->path, must_open);
    if (!s->fp) return;
    /* what the sequential reader has to take: rest[0 .. n_rest), then the stream */
    char first = 0;
    const char *rest = &first, *how = getenv("CORNETTO_FASTQ_SPLIT");
    size_t n_rest = gzread(s->fp, &first, 1) == 1;
    int more = n_rest != 0;
    const int host = (how && !strcmp(how, "host")) || (s->names_only && cli_host_mode()); /* the sequential reader alone (CORNETTO_ACCEL=no: no device) */
    s->size = s->raw_fd = -1;
    if (n_rest && (first == '@' || first == '>') && !host) {
        const int fasta = first == '>';
        struct stat st;
        if (strcmp(s->path, "-") && gzdirect(s->fp) && stat(s->path, &st) == 0 && S_ISREG(st.st_mode)) {
            s->size = (int64_t)st.st_size;
            s->raw_fd = open(s->path, O_RDONLY);
        }
        if (fasta && s->raw_fd >= 0 && s->warm && s->size >= (256LL << 20)) cli_accel_warm_hint(s->warm); /* (an assembly: its one scan should not be the runtime's first) */
        if (!s->h) cli_accel_open_begin();
        /* CORNETTO_CLI_WHOLE=0 and an explicit piece size keep the piece loop */
        const char *we = getenv("CORNETTO_CLI_WHOLE");
        const int whole = !(we && !atoi(we)) && !getenv("CORNETTO_FASTQ_PIECE");
        /* a compressed regular file: bgzip's output is inflated on the device (CORNETTO_BGZF=0: never) */
        const char *be = getenv("CORNETTO_BGZF");
        int64_t bz_resume = 0, bz_total = 0;
        int bz = 0;
        if (whole && s->raw_fd < 0 && strcmp(s->path, "-") && !gzdirect(s->fp) && !(be && !atoi(be)) && stat(s->path, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            const int fd = open(s->path, O_RDONLY);
            const int is_bgzf = fd >= 0 && cli_bgzf_first_member(fd);
            if (fd >= 0) close(fd);
            if (!is_bgzf) bgzf_fallback(s, "not BGZF");
            else if (!fasta) bgzf_fallback(s, "not FASTA");
            else bz = stream_bgzf_fasta(s, (int64_t)st.st_size, &bz_resume, &bz_total);
        }
        if (bz) {
            n_rest = 0;
            more = bz_resume < bz_total;
            if (more) bgzf_fallback(s, "the text is not plain FASTA to its end: the sequential reader goes on");
            if (more) gzseek(s->fp, (z_off_t)bz_resume, SEEK_SET);
        } else if (fasta && s->raw_fd >= 0 && s->size > 0 && whole) {
            const int64_t resume = stream_whole_fasta(s);
            close(s->raw_fd);
            n_rest = 0;
            more = resume < s->size;
            if (more) gzseek(s->fp, (z_off_t)resume, SEEK_SET);
        } else {
            more = stream_pieces(s, first, &rest, &n_rest);
        }
    }
    if (more) stream_sequential(s, rest, n_rest);
    else gzclose(s->fp);
    stream_release(s);
    TRACE("done");
}

void stream_records(const char *path, int must_open, scan_fn scan, void *arg, int warm)
{
    stream_t s = {.path = path, .scan = scan, .arg = arg, .warm = warm};
    stream_run(&s, must_open);
}

/* for a sub-command that reads several files (qv): the caller's handle, and what the call allocated goes before it returns */
void stream_records_on(cornetto_accel_t *h, const char *path, int must_open, scan_fn scan, void *arg)
{
    stream_t s = {.path = path, .scan = scan, .arg = arg, .release = 1, .h = h};
    stream_run(&s, must_open);
}

/* one device handle serves every stream_names() call of the process */
static cornetto_accel_t *g_names_h;

void stream_names(const char *path, int must_open, scan_fn names, void *arg)
{
    stream_t s = {.path = path, .scan = names, .arg = arg, .names_only = 1, .h = g_names_h};
    stream_run(&s, must_open);
    g_names_h = s.h;
}
