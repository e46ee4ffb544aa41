// bamfq_sim.cc — the size pass and the text kernel of `seq --bam` (cornetto_amd/csrc/bamfq.hpp, with the header and record chain of
// bam.hpp) on the CPU.  The same statements as in bamfq_size / bamfq_text, one thread of control after the other; the text of every window,
// the record offsets, the size and offset tables and the bytes of every get live in heap blocks of exactly their size, so that the host
// sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/bamfq_sim.cc -lz -o bamfq_sim
//   bamfq_sim [--window W] [--range R] [--min-len N] [--duplex] cases.bin
// cases.bin: any number of { u32 n, n bytes: the inflated bytes of a BAM (valid, mutated or cut short) }.  Every case is taken through the
// windows of bamfq.hip's feed — W bytes of the file behind the tail the last window left, the whole file by default — and every window's text
// is fetched as the gets of the device fetch it: a first range of 7 bytes, then ranges of R bytes (the whole text by default), so that `at`
// is no multiple of 16, each cut into the kernel's tiles and 16-byte chunks.  One line per case:
//   status kind record a b text_bytes crc32(text) [total_reads total_bases kept_reads kept_bases]
// which tests/test_bamfq_host.py compares with the oracle's (tests/bamfq_cases.py).  Exit 0 and no sanitizer report: the argument for the
// bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include <vector>

#include "../../cornetto_amd/csrc/bamfq.hpp"

static const int64_t TILE = 16384;      // bamfq.hip: FQ_TILE

struct Answer {
    int status = 0, kind = 0;
    long long record = 0, a = 0, b = 0, stats[4] = {0, 0, 0, 0};
    std::vector<uint8_t> text;
};

static void fail(Answer &r, int kind, long long record, long long a, long long b)
{
    r.status = CORNETTO_E_FORMAT;
    r.kind = kind;
    r.record = record;
    r.a = a;
    r.b = b;
}

// bytes [at, at + n) of the window's text as bamfq_text writes them, appended to `to`
static void get(const CnqSrc &S, int64_t at, int64_t n, std::vector<uint8_t> &to)
{
    uint8_t *dst = (uint8_t *)malloc((size_t)n);
    for (int64_t tile = 0; tile < n; tile += TILE) {
        const int64_t t_end = n - tile < TILE ? n - tile : TILE;
        const int64_t r0 = cnq_find(S.out, 0, S.n - 1, at + tile);
        const int64_t r1 = cnq_find(S.out, r0, S.n - 1, at + tile + t_end - 1);
        for (int64_t rel = tile; rel < tile + t_end; rel += 16) {
            const int m = (int)(n - rel < 16 ? n - rel : 16);
            uint64_t v[2];
            cnq_chunk(S, r0, r1, at + rel, m, v);
            memcpy(dst + rel, v, (size_t)m);      // (the device stores all 16 bytes: its slab is rounded up)
        }
    }
    to.insert(to.end(), dst, dst + n);
    free(dst);
}

static Answer run(const uint8_t *file, int64_t n, int64_t window, int64_t range, int32_t min_len, int duplex)
{
    Answer ans;
    int32_t n_ref = 0, *lens = nullptr;
    char **names = nullptr;
    int64_t hdr = 0;
    {
        uint8_t *exact = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0) memcpy(exact, file, (size_t)n);
        const int rc = cnb_header(exact, n, &n_ref, &names, &lens, &hdr);
        free(exact);
        if (rc == 1) { fail(ans, CNB_TRUNC, -1, 0, -1); return ans; }
        if (rc != CORNETTO_OK) { fail(ans, 7, -1, 0, 0); return ans; }
        for (int32_t i = 0; i < n_ref; ++i) free(names[i]);
        free(names);
        free(lens);
    }
    std::vector<uint8_t> tail;
    int64_t fed = 0, skip = hdr, n_records = 0;
    bool stop = false;
    while (!stop && (fed < n || fed == 0)) {
        const int64_t take = window > 0 ? (window < n - fed ? window : n - fed) : n - fed;
        const int64_t n_text = (int64_t)tail.size() + take;
        uint8_t *text = (uint8_t *)malloc(n_text > 0 ? (size_t)n_text : 1);
        if (!tail.empty()) memcpy(text, tail.data(), tail.size());
        if (take > 0) memcpy(text + tail.size(), file + fed, (size_t)take);
        fed += take;
        const int64_t start = skip < n_text ? skip : n_text;
        skip -= start;
        const int64_t cap = (n_text - start) / 36 + 1;
        uint32_t *rec_off = (uint32_t *)malloc((size_t)cap * 4);
        int64_t end = 0;
        int32_t ferr = 0, ferr_a = 0;
        const int64_t k = cnb_frame(text, start, n_text, rec_off, cap, &end, &ferr, &ferr_a);
        uint32_t *size = (uint32_t *)malloc(k > 0 ? (size_t)k * 4 : 1);
        int64_t n_ok = k;
        CnbErr bad{0, 0, 0};
        std::vector<CnqOut> outs((size_t)k);
        for (int64_t r = 0; r < k; ++r) {      // (the device runs every record of the window: so does this, the first failure decides)
            CnbErr e;
            const int kind = cnq_size(text + rec_off[r], n_ref, min_len, duplex, outs[(size_t)r], e);
            size[r] = kind == CNB_OK ? outs[(size_t)r].size : 0u;
            if (kind != CNB_OK && n_ok == k) {
                n_ok = r;
                bad = e;
            }
        }
        uint32_t *out = (uint32_t *)malloc(((size_t)n_ok + 1) * 4);
        uint64_t sum = 0;
        for (int64_t r = 0; r < n_ok; ++r) {
            out[r] = (uint32_t)sum;
            sum += size[r];
            if (outs[(size_t)r].kept >= 0) {
                ans.stats[0] += 1;
                ans.stats[1] += outs[(size_t)r].l_seq;
                if (outs[(size_t)r].kept) {
                    ans.stats[2] += 1;
                    ans.stats[3] += outs[(size_t)r].l_seq;
                }
            }
        }
        out[n_ok] = (uint32_t)sum;
        const CnqSrc S{text, rec_off, out, n_ok};
        const int64_t total = (int64_t)sum;
        for (int64_t at = 0; at < total;) {
            int64_t m = at == 0 ? 7 : (range > 0 ? range : total);
            if (m > total - at) m = total - at;
            get(S, at, m, ans.text);
            at += m;
        }
        if (n_ok < k) {
            fail(ans, bad.kind, n_records + n_ok, bad.a, bad.b);
            stop = true;
        } else {
            n_records += k;
            if (ferr != CNB_OK) {
                fail(ans, ferr, n_records, ferr_a, 0);
                stop = true;
            }
        }
        tail.assign(text + end, text + n_text);
        free(out);
        free(size);
        free(rec_off);
        free(text);
        if (take == 0) break;
    }
    if (!stop && !tail.empty()) fail(ans, CNB_TRUNC, n_records, (long long)tail.size(), tail.size() >= 4 ? (long long)(int32_t)cnb_u32(tail.data()) : -1);
    return ans;
}

int main(int argc, char **argv)
{
    int64_t window = 0, range = 0;
    int32_t min_len = 0;
    int duplex = 0;
    const char *path = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--window") && i + 1 < argc) window = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--range") && i + 1 < argc) range = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-len") && i + 1 < argc) min_len = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--duplex")) duplex = 1;
        else path = argv[i];
    }
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) { fprintf(stderr, "usage: bamfq_sim [--window W] [--range R] [--min-len N] [--duplex] cases.bin\n"); return 1; }
    for (;;) {
        uint8_t h[4];
        if (fread(h, 1, 4, f) != 4) break;
        const uint32_t n = cnb_u32(h);
        std::vector<uint8_t> buf(n);
        if (n && fread(buf.data(), 1, n, f) != n) { fprintf(stderr, "cases file cut short\n"); return 1; }
        const Answer r = run(buf.data(), (int64_t)n, window, range, min_len, duplex);
        const unsigned long crc = crc32(crc32(0L, Z_NULL, 0), r.text.data(), (uInt)r.text.size());
        if (r.status) printf("%d %d %lld %lld %lld %zu %lu\n", r.status, r.kind, r.record, r.a, r.b, r.text.size(), crc);
        else printf("0 0 0 0 0 %zu %lu %lld %lld %lld %lld\n", r.text.size(), crc, r.stats[0], r.stats[1], r.stats[2], r.stats[3]);
    }
    fclose(f);
    return 0;
}
