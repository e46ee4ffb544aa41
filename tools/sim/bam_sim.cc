// bam_sim.cc — the BAM header, record chain and record / CIGAR walk of the device path (cornetto_amd/csrc/bam.hpp) on the CPU.
// The same statements as in bam_frame / bam_depth with the 64 lanes run one after the other; the text of every window, the record
// offsets and the difference arrays live in heap blocks of exactly their size, so that the host sanitizers see every byte read or
// written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/bam_sim.cc -lz -o bam_sim
//   bam_sim [--window W] [--mapq N] cases.bin
// cases.bin: any number of { u32 n, n bytes: the inflated bytes of a BAM (valid, mutated or cut short) }.  Every case is taken through the
// windows of bam.hip's feed — W bytes of the file behind the tail the last window left, the whole file by default — and answered with one line
//   status kind record a b n_records n_counted n_clamped crc32(total depths) crc32(mq depths)
// which tests/test_bam_host.py compares with the oracle's (tests/bam_cases.py).  Exit 0 and no sanitizer report: the argument for the
// bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include <vector>

#include "../../cornetto_amd/csrc/bam.hpp"

struct HostLanes {
    static constexpr int SLOTS = 64;
    static int first() { return 0; }
    static int step() { return 1; }
    static int slot(int l) { return l; }
    static bool leader() { return true; }
    static void scan(unsigned long long (&v)[64])
    {
        for (int i = 1; i < 64; ++i) v[i] += v[i - 1];
    }
    static unsigned long long last(const unsigned long long (&v)[64]) { return v[63]; }
    static unsigned long long sum(const unsigned long long (&v)[64])
    {
        unsigned long long s = 0;
        for (int i = 0; i < 64; ++i) s += v[i];
        return s;
    }
};

// heap blocks of exactly n elements: the sanitizer's red zones begin behind the last one
struct Sink {
    int32_t *tot, *mq;
    int64_t n;
    long bad = 0;
    void add(int64_t i, int d, bool q)
    {
        tot[i] += d;          // (an index outside the block is the sanitizer's to report)
        if (q) mq[i] += d;
    }
};

struct Answer {
    int status = 0, kind = 0;
    long long record = 0, a = 0, b = 0, n_records = 0, n_counted = 0, n_clamped = 0;
    unsigned long crc_t = 0, crc_q = 0;
};

static Answer fail(int kind, long long record, long long a, long long b)
{
    Answer r;
    r.status = CORNETTO_E_FORMAT;
    r.kind = kind;
    r.record = record;
    r.a = a;
    r.b = b;
    return r;
}

static Answer run(const uint8_t *file, int64_t n, int64_t window, int32_t min_mapq)
{
    int32_t n_ref = 0, *lens = nullptr;
    char **names = nullptr;
    int64_t hdr = 0;
    {
        uint8_t *exact = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0) memcpy(exact, file, (size_t)n);
        const int rc = cnb_header(exact, n, &n_ref, &names, &lens, &hdr);
        free(exact);
        if (rc == 1) return fail(CNB_TRUNC, -1, 0, -1);
        if (rc != CORNETTO_OK) return fail(7, -1, 0, 0);
    }
    std::vector<int64_t> off((size_t)n_ref);
    int64_t pos = 0;
    for (int32_t i = 0; i < n_ref; ++i) {
        off[(size_t)i] = pos;
        pos = (pos + lens[i] + 63) / 64 * 64;
    }
    const int64_t n_el = (n_ref ? off[(size_t)n_ref - 1] + lens[n_ref - 1] : 0) + 1;      // the last contig's end and the pad element, nothing more
    Sink sink{(int32_t *)calloc((size_t)n_el, 4), (int32_t *)calloc((size_t)n_el, 4), n_el};
    int32_t *len_x = (int32_t *)malloc((size_t)(n_ref ? n_ref : 1) * 4);
    int64_t *off_x = (int64_t *)malloc((size_t)(n_ref ? n_ref : 1) * 8);
    for (int32_t i = 0; i < n_ref; ++i) { len_x[i] = lens[i]; off_x[i] = off[(size_t)i]; }
    const CnbRefs R{n_ref, len_x, off_x};
    Answer ans;
    std::vector<uint8_t> tail;
    int64_t fed = 0, skip = hdr;
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
        for (int64_t r = 0; r < k && !stop; ++r) {
            CnbOut o;
            CnbErr e;
            if (cnb_record<HostLanes>(text + rec_off[r], R, min_mapq, 0x704u, sink, o, e) != CNB_OK) {
                ans = fail(e.kind, ans.n_records + r, e.a, e.b);
                stop = true;
            } else {
                ans.n_counted += o.counted;
            }
        }
        if (!stop) {
            ans.n_records += k;
            if (ferr != CNB_OK) {
                ans = fail(ferr, ans.n_records, ferr_a, 0);
                stop = true;
            }
        }
        tail.assign(text + end, text + n_text);
        free(rec_off);
        free(text);
        if (take == 0) break;
    }
    if (!stop && !tail.empty()) {
        ans = fail(CNB_TRUNC, ans.n_records, (long long)tail.size(), tail.size() >= 4 ? (long long)(int32_t)cnb_u32(tail.data()) : -1);
        stop = true;
    }
    if (!stop) {      // the scan: every contig sums to zero, every prefix is a depth
        for (int q = 0; q < 2; ++q) {
            const int32_t *d = q ? sink.mq : sink.tot;
            unsigned long crc = crc32(0L, Z_NULL, 0);
            int64_t run_sum = 0, at = 0;
            for (int32_t c = 0; c < n_ref; ++c) {
                for (; at < off[(size_t)c]; ++at) run_sum += d[at];
                std::vector<uint16_t> out((size_t)lens[c]);
                for (int32_t i = 0; i < lens[c]; ++i, ++at) {
                    run_sum += d[at];
                    if (run_sum < 0) { fprintf(stderr, "FAIL: negative depth at contig %d position %d\n", c, i); exit(2); }
                    if (run_sum > 65535) ++ans.n_clamped;
                    out[(size_t)i] = (uint16_t)(run_sum > 65535 ? 65535 : run_sum);
                }
                if (!out.empty()) crc = crc32(crc, (const Bytef *)out.data(), (uInt)(out.size() * 2));
            }
            for (; at < n_el; ++at) run_sum += d[at];
            if (run_sum != 0) { fprintf(stderr, "FAIL: the difference array sums to %lld\n", (long long)run_sum); exit(2); }
            (q ? ans.crc_q : ans.crc_t) = crc;
        }
    }
    free(sink.tot); free(sink.mq); free(len_x); free(off_x);
    for (int32_t i = 0; i < n_ref; ++i) free(names[i]);
    free(names); free(lens);
    return ans;
}

int main(int argc, char **argv)
{
    int64_t window = 0;
    int32_t min_mapq = 20;
    const char *path = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--window") && i + 1 < argc) window = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--mapq") && i + 1 < argc) min_mapq = atoi(argv[++i]);
        else path = argv[i];
    }
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) { fprintf(stderr, "usage: bam_sim [--window W] [--mapq N] cases.bin\n"); return 1; }
    for (;;) {
        uint8_t h[4];
        if (fread(h, 1, 4, f) != 4) break;
        const uint32_t n = cnb_u32(h);
        std::vector<uint8_t> buf(n);
        if (n && fread(buf.data(), 1, n, f) != n) { fprintf(stderr, "cases file cut short\n"); return 1; }
        const Answer r = run(buf.data(), (int64_t)n, window, min_mapq);
        printf("%d %d %lld %lld %lld %lld %lld %lld %lu %lu\n", r.status, r.kind, r.record, r.a, r.b, r.n_records, r.n_counted, r.n_clamped, r.crc_t, r.crc_q);
    }
    fclose(f);
    return 0;
}
