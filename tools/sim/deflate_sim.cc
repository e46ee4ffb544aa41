// deflate_sim.cc — the device's BGZF encoder (cornetto_amd/csrc/deflate.hpp) on the CPU, against zlib.  The same statements as in
// bgzf_deflate with the 64 lanes run one after the other; the source bytes of a member live in a heap block of exactly their number and the
// staging in one of exactly CND_STRIDE bytes, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/deflate_sim.cc -lz -o deflate_sim
//   deflate_sim file ...
// Every file is cut every CND_MEMBER bytes and every piece made a member, twice: over a staging block filled with 0x00 and one filled with
// 0xA5 — the same bytes must come out.  zlib's raw inflate must end the member's stream with the piece's bytes, BSIZE, CRC-32 and ISIZE must
// be theirs and the size at most CND_MAX_SIZE; the chain walk of inflate.hpp must take the members.  The chain is written to FILE.bgzf
// (without the end-of-file block).  Exit 0 and no sanitizer report: the argument for the bounds of the kernel.
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../../cornetto_amd/csrc/deflate.hpp"

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
    static uint64_t ballot(const bool *f)
    {
        uint64_t m = 0;
        for (int l = 0; l < 64; ++l) m |= (uint64_t)(f[l] ? 1 : 0) << l;
        return m;
    }
    static uint32_t scan(const uint32_t *v, uint32_t *ex)
    {
        uint32_t s = 0;
        for (int l = 0; l < 64; ++l) {
            ex[l] = s;
            s += v[l];
        }
        return s;
    }
    static uint32_t pick(const uint32_t *v, int lane) { return v[lane & 63]; }
    static void lds_or(uint32_t *p, uint32_t v) { *p |= v; }
    static void lds_add(uint32_t *p, uint32_t v) { *p += v; }
};

static long g_fail;

static int one_member(const uint8_t *piece, int32_t n, int fill, std::vector<uint8_t> &member, const char *what)
{
    uint8_t *src = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
    if (n > 0) memcpy(src, piece, (size_t)n);
    uint8_t *out = (uint8_t *)malloc(CND_STRIDE);
    memset(out, fill, CND_STRIDE);
    static CndShared sh;
    memset(&sh, fill, sizeof(sh));
    const int32_t size = cnd_member<HostLanes>(n > 0 ? src : src + 1, n, out, sh);
    int bad = 0;
    if (size < 26 || size > CND_MAX_SIZE) {
        fprintf(stderr, "FAIL %s: a member of %d bytes\n", what, size);
        bad = 1;
    } else {
        member.assign(out + CND_HEAD, out + CND_HEAD + size);
        CniMember m;
        if (cni_bgzf_member(member.data(), size, &m) != 1 || m.size != size || m.payload != 18) {
            fprintf(stderr, "FAIL %s: not a BGZF member of %d bytes\n", what, size);
            bad = 1;
        } else {
            std::vector<uint8_t> ref((size_t)n + 1);
            z_stream z;
            memset(&z, 0, sizeof(z));
            inflateInit2(&z, -15);
            z.next_in = member.data() + 18;
            z.avail_in = (uInt)(size - 26);
            z.next_out = ref.data();
            z.avail_out = (uInt)ref.size();
            const int zr = inflate(&z, Z_FINISH);
            const bool good = zr == Z_STREAM_END && (int64_t)z.total_out == n && z.avail_in == 0 && (n == 0 || memcmp(ref.data(), src, (size_t)n) == 0) &&
                              m.isize == (uint32_t)n && m.crc == (uint32_t)crc32(0L, src, (uInt)n);
            inflateEnd(&z);
            if (!good) {
                fprintf(stderr, "FAIL %s: zlib %d, %lu of %d bytes, %u input bytes left, CRC %08x ISIZE %u\n", what, zr, z.total_out, n, z.avail_in, m.crc, m.isize);
                bad = 1;
            }
        }
    }
    free(src);
    free(out);
    g_fail += bad;
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: deflate_sim file ...\n");
        return 2;
    }
    long n_members = 0;
    for (int a = 1; a < argc; ++a) {
        const char *path = argv[a];
        FILE *f = fopen(path, "rb");
        if (!f) { perror(path); return 2; }
        std::vector<uint8_t> all;
        static uint8_t tmp[65536];
        size_t g;
        while ((g = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + g);
        fclose(f);
        std::vector<uint8_t> chain;
        for (size_t at = 0; at < all.size(); at += CND_MEMBER, ++n_members) {
            const int32_t n = (int32_t)(all.size() - at < CND_MEMBER ? all.size() - at : CND_MEMBER);
            char what[512];
            snprintf(what, sizeof(what), "%s member at %zu", path, at);
            std::vector<uint8_t> m0, m1;
            if (one_member(all.data() + at, n, 0x00, m0, what) || one_member(all.data() + at, n, 0xA5, m1, what)) continue;
            if (m0 != m1) {
                fprintf(stderr, "FAIL %s: the member depends on what its memory held before\n", what);
                ++g_fail;
            }
            chain.insert(chain.end(), m0.begin(), m0.end());
        }
        // the chain walk takes what was made
        std::vector<cornetto_bgzf_block_t> blocks(chain.size() / 26 + 2);
        int64_t dst = 0, nb = 0, resume = 0;
        int32_t broken = 0;
        if (!chain.empty()) cni_bgzf_scan(chain.data(), (int64_t)chain.size(), 0, &dst, blocks.data(), (int64_t)blocks.size(), &nb, &resume, &broken);
        if (broken || resume != (int64_t)chain.size() || (g_fail == 0 && dst != (int64_t)all.size())) {
            fprintf(stderr, "FAIL %s: the chain of %zu bytes is walked to %lld, %lld bytes inflated of %zu\n", path, chain.size(), (long long)resume, (long long)dst, all.size());
            ++g_fail;
        }
        const std::string o = std::string(path) + ".bgzf";
        FILE *w = fopen(o.c_str(), "wb");
        if (!w || (!chain.empty() && fwrite(chain.data(), 1, chain.size(), w) != chain.size()) || fclose(w) != 0) { perror(o.c_str()); return 2; }
        printf("%s\t%zu\t%zu\n", path, all.size(), chain.size());
    }
    printf("deflate_sim: %ld members, %ld failures\n", n_members, g_fail);
    return g_fail ? 1 : 0;
}
