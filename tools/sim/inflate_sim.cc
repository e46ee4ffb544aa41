// inflate_sim.cc — the device's deflate decoder, CRC-32 and BGZF chain walk (cornetto_amd/csrc/inflate.hpp) on the CPU, against zlib.
// The same statements as in bgzf_inflate / bgzf_crc32 with the 64 lanes run one after the other; input and output live in heap blocks
// of exactly n_src and n_dst bytes, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/inflate_sim.cc -lz -o inflate_sim
//   inflate_sim [--mut N] [--seed S] [--status] file.gz ...
// For every BGZF member of every file: the member as it is, N seeded single-bit and single-byte changes of its deflate stream, the
// stream cut short (n_src smaller by 1, 2, 3, 4, 8, to a half, to nothing) and n_dst one lower and one higher.  The rule of every trial:
// where zlib's raw inflate ends the stream with exactly n_dst bytes whose CRC-32 is the footer's, the decoder returns the same bytes and
// the CRC agrees; in every other case the decoder reports the block bad.  The chain walk is run over every file cut into two pieces at
// seeded offsets.  Exit 0 and no sanitizer report: the argument for the bounds of the kernels.  --status: one line `status <file> <member> <code>`
// for every member's as-it-is trial, the CNI_* code the decoder and the CRC check gave it (the tests pin the reason of every bad stream).
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include <vector>

#include "../../cornetto_amd/csrc/inflate.hpp"

struct HostLanes {
    static constexpr int SLOTS = 64;
    static int first() { return 0; }
    static int step() { return 1; }
    static int slot(int l) { return l; }
    static bool leader() { return true; }
    static void sync() {}
    static int uni(int v) { return v; }
    static uint32_t uni(uint32_t v) { return v; }
    static void put(uint8_t *lit, int lane, uint8_t v) { lit[lane] = v; }
};

static uint64_t g_rng = 1;
static uint32_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

static long g_trials, g_good, g_fail;

// one trial -> 0 when the rule holds; *status: the CNI_* code of the trial
static int trial(const uint8_t *payload, int32_t n_src, int32_t n_dst, uint32_t crc, const char *what, int *status = nullptr)
{
    uint8_t *src = (uint8_t *)malloc(n_src > 0 ? (size_t)n_src : 1);     // exact sizes: the sanitizer's red zones begin at the last byte
    if (n_src > 0) memcpy(src, payload, (size_t)n_src);
    uint8_t *dst = (uint8_t *)calloc(1, n_dst > 0 ? (size_t)n_dst : 1);
    static CniShared sh;
    static uint32_t tab[4 * 256], red[64];
    int st = cni_inflate<HostLanes>(src, n_src, n_dst > 0 ? dst : dst + 1, n_dst, sh);
    uint32_t got_crc = 0;
    if (st == CNI_OK) {
        got_crc = cni_crc32<HostLanes>(dst, n_dst, tab, red);
        if (got_crc != (uint32_t)crc32(0L, dst, (uInt)n_dst)) {
            fprintf(stderr, "FAIL %s: CRC-32 %08x, zlib's is %08lx\n", what, got_crc, crc32(0L, dst, (uInt)n_dst));
            ++g_fail;
        }
        if (got_crc != crc) st = CNI_BAD_CRC;
    }
    if (status) *status = st;
    // zlib's raw inflate on the same bytes, with room for one byte more than n_dst
    std::vector<uint8_t> ref((size_t)n_dst + 1);
    z_stream z;
    memset(&z, 0, sizeof(z));
    inflateInit2(&z, -15);
    z.next_in = src;
    z.avail_in = (uInt)n_src;
    z.next_out = ref.data();
    z.avail_out = (uInt)ref.size();
    const int zr = inflate(&z, Z_FINISH);
    const bool zgood = zr == Z_STREAM_END && (int64_t)z.total_out == n_dst && (uint32_t)crc32(0L, ref.data(), (uInt)n_dst) == crc;
    inflateEnd(&z);
    int bad = 0;
    if (zgood) {
        if (st != CNI_OK || memcmp(dst, ref.data(), (size_t)n_dst) != 0) bad = 1;
        ++g_good;
    } else if (st == CNI_OK) {
        bad = 1;
    }
    if (bad) {
        fprintf(stderr, "FAIL %s: n_src %d n_dst %d: zlib %s (%d, %lu bytes), decoder status %d\n", what, n_src, n_dst, zgood ? "good" : "bad", zr, z.total_out, st);
        ++g_fail;
    }
    ++g_trials;
    free(src);
    free(dst);
    return bad;
}

int main(int argc, char **argv)
{
    long n_mut = 200;
    bool print_status = false;
    std::vector<const char *> files;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--mut") && i + 1 < argc) n_mut = atol(argv[++i]);
        else if (!strcmp(argv[i], "--seed") && i + 1 < argc) g_rng = strtoull(argv[++i], NULL, 10) * 2 + 1;
        else if (!strcmp(argv[i], "--status")) print_status = true;
        else files.push_back(argv[i]);
    }
    if (files.empty()) {
        fprintf(stderr, "usage: inflate_sim [--mut N] [--seed S] [--status] file.gz ...\n");
        return 2;
    }
    long n_members = 0;
    for (const char *path : files) {
        FILE *f = fopen(path, "rb");
        if (!f) { perror(path); return 2; }
        std::vector<uint8_t> all;
        uint8_t tmp[65536];
        size_t g;
        while ((g = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + g);
        fclose(f);
        const int64_t n = (int64_t)all.size();
        // the chain in one go
        std::vector<cornetto_bgzf_block_t> blocks((size_t)(n / 26 + 2));
        int64_t dst = 0, nb = 0, resume = 0;
        int32_t broken = 0;
        uint8_t *exact = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
        memcpy(exact, all.data(), (size_t)n);
        cni_bgzf_scan(exact, n, 0, &dst, blocks.data(), (int64_t)blocks.size(), &nb, &resume, &broken);
        // ... and cut in two at seeded offsets: the same blocks, whatever the cut
        for (int k = 0; k < 64 && n > 0; ++k) {
            const int64_t cut = (int64_t)(rnd() % (uint64_t)(n + 1));
            std::vector<cornetto_bgzf_block_t> b2(blocks.size());
            int64_t d2 = 0, n1 = 0, n2 = 0, r1 = 0, r2 = 0;
            int32_t br1 = 0, br2 = 0;
            uint8_t *head = (uint8_t *)malloc(cut > 0 ? (size_t)cut : 1);
            memcpy(head, exact, (size_t)cut);
            cni_bgzf_scan(head, cut, 0, &d2, b2.data(), (int64_t)b2.size(), &n1, &r1, &br1);
            free(head);
            if (!br1) {
                uint8_t *tail = (uint8_t *)malloc(n - r1 > 0 ? (size_t)(n - r1) : 1);
                memcpy(tail, exact + r1, (size_t)(n - r1));
                cni_bgzf_scan(tail, n - r1, r1, &d2, b2.data() + n1, (int64_t)b2.size() - n1, &n2, &r2, &br2);
                free(tail);
            } else {
                r2 = r1;
                br2 = 1;
            }
            if (n1 + n2 != nb || r2 != resume || br2 != broken || d2 != dst || memcmp(b2.data(), blocks.data(), (size_t)nb * sizeof(cornetto_bgzf_block_t)) != 0) {
                fprintf(stderr, "FAIL %s: the chain cut at %lld differs (%lld + %lld blocks of %lld, resume %lld of %lld)\n", path, (long long)cut, (long long)n1, (long long)n2,
                        (long long)nb, (long long)r2, (long long)resume);
                ++g_fail;
            }
        }
        for (int64_t i = 0; i < nb; ++i, ++n_members) {
            const cornetto_bgzf_block_t &B = blocks[(size_t)i];
            const uint8_t *p = exact + B.src;
            char what[512];
            snprintf(what, sizeof(what), "%s member %lld as it is", path, (long long)i);
            int st = -1;
            const int failed = trial(p, B.n_src, B.n_dst, B.crc, what, &st);
            if (print_status) printf("status %s %lld %d\n", path, (long long)i, st);
            if (failed) continue;
            static const int cuts[] = {1, 2, 3, 4, 8};
            for (int c : cuts)
                if (B.n_src >= c) {
                    snprintf(what, sizeof(what), "%s member %lld n_src - %d", path, (long long)i, c);
                    trial(p, B.n_src - c, B.n_dst, B.crc, what);
                }
            snprintf(what, sizeof(what), "%s member %lld n_src halved", path, (long long)i);
            trial(p, B.n_src / 2, B.n_dst, B.crc, what);
            trial(p, 0, B.n_dst, B.crc, what);
            snprintf(what, sizeof(what), "%s member %lld n_dst + 1", path, (long long)i);
            trial(p, B.n_src, B.n_dst + 1, B.crc, what);
            if (B.n_dst > 0) {
                snprintf(what, sizeof(what), "%s member %lld n_dst - 1", path, (long long)i);
                trial(p, B.n_src, B.n_dst - 1, B.crc, what);
            }
            std::vector<uint8_t> m(p, p + B.n_src);
            for (long k = 0; k < n_mut && B.n_src > 0; ++k) {
                // half of the changes in the first 64 bytes, where the block header and the code lengths are
                const uint32_t span = (k & 1) && B.n_src > 64 ? 64u : (uint32_t)B.n_src;
                const uint32_t at = rnd() % span;
                const uint8_t old = m[at];
                if (k & 2) m[at] = (uint8_t)(old ^ (1u << (rnd() & 7)));
                else m[at] = (uint8_t)(old + 1 + rnd() % 255);
                snprintf(what, sizeof(what), "%s member %lld byte %u %02x -> %02x", path, (long long)i, at, old, m[at]);
                trial(m.data(), B.n_src, B.n_dst, B.crc, what);
                m[at] = old;
            }
        }
        free(exact);
    }
    printf("inflate_sim: %ld members, %ld trials (%ld of them good for zlib), %ld failures\n", n_members, g_trials, g_good, g_fail);
    return g_fail ? 1 : 0;
}
