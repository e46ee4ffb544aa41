/* bgzf_out.c — `seq --bam --bgzf` on the host: stdout as a BGZF stream (an extension; include/cornetto_accel.h states the member a device call
 * makes: cornetto_text_deflate).  Text is collected 65280 bytes at a time, deflated raw by zlib and wrapped as bgzip wraps it; members that
 * the device made go out as they are, behind whatever text is pending, so that a file whose reading moves from the device to the host in its
 * middle stays one stream.  The stream ends with the 28-byte end-of-file block only on success: a reader tells a cut file by its absence. */
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "cli.h"

#define BGZF_OUT_MEMBER 65280

static int bgzf_out_on;
static size_t bgzf_out_n;
static unsigned char *bgzf_out_text, *bgzf_out_comp;

static void bgzf_out_put(const void *p, size_t n)
{
    if (n && fwrite(p, 1, n, stdout) != n) {
        CLI_ERROR("%s", "cannot write to the standard output");
        exit(EXIT_FAILURE);
    }
}

void cli_bgzf_out_begin(void)
{
    bgzf_out_on = 1;
    bgzf_out_n = 0;
    if (!bgzf_out_text) {
        bgzf_out_text = (unsigned char *)cli_xmalloc(BGZF_OUT_MEMBER);
        bgzf_out_comp = (unsigned char *)cli_xmalloc(65536);
    }
}

int cli_bgzf_out_active(void) { return bgzf_out_on; }

/* the pending text as one member (nothing pending: nothing) */
void cli_bgzf_out_flush(void)
{
    if (!bgzf_out_on || bgzf_out_n == 0) return;
    const size_t n = bgzf_out_n;
    unsigned char *o = bgzf_out_comp;
    size_t pay = 0;
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK) {
        z.next_in = bgzf_out_text;
        z.avail_in = (uInt)n;
        z.next_out = o + 18;
        z.avail_out = (uInt)(n + 4);      /* smaller than a stored block, or stored */
        if (deflate(&z, Z_FINISH) == Z_STREAM_END) pay = (size_t)z.total_out;
        deflateEnd(&z);
    }
    if (pay == 0) {
        o[18] = 1;
        o[19] = (unsigned char)n;
        o[20] = (unsigned char)(n >> 8);
        o[21] = (unsigned char)~n;
        o[22] = (unsigned char)(~n >> 8);
        memcpy(o + 23, bgzf_out_text, n);
        pay = n + 5;
    }
    static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    const size_t size = 18 + pay + 8;
    const unsigned long crc = crc32(crc32(0L, Z_NULL, 0), bgzf_out_text, (uInt)n);
    memcpy(o, head, 16);
    o[16] = (unsigned char)(size - 1);
    o[17] = (unsigned char)((size - 1) >> 8);
    for (int k = 0; k < 4; ++k) {
        o[18 + pay + k] = (unsigned char)(crc >> (8 * k));
        o[22 + pay + k] = (unsigned char)(n >> (8 * k));
    }
    bgzf_out_n = 0;
    bgzf_out_put(o, size);
}

void cli_bgzf_out_text(const void *p, size_t n)
{
    const unsigned char *s = (const unsigned char *)p;
    while (n) {
        const size_t k = n < BGZF_OUT_MEMBER - bgzf_out_n ? n : BGZF_OUT_MEMBER - bgzf_out_n;
        memcpy(bgzf_out_text + bgzf_out_n, s, k);
        bgzf_out_n += k;
        s += k;
        n -= k;
        if (bgzf_out_n == BGZF_OUT_MEMBER) cli_bgzf_out_flush();
    }
}

void cli_bgzf_out_members(const void *p, size_t n)
{
    cli_bgzf_out_flush();
    bgzf_out_put(p, n);
}

void cli_bgzf_out_end(void)
{
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    cli_bgzf_out_flush();
    bgzf_out_put(eof, sizeof(eof));
    bgzf_out_on = 0;
}
