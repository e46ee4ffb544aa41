// bgsrc_sim.cc — the index arithmetic of a compressed bedgraph source (csrc/bgtok.hpp: bgsrc_size, bgsrc_inflate, bg_names) as a
// CPU program under the host sanitizers: every buffer is a heap block of exactly the size the library asks for, so an index that leaves its
// buffer is an AddressSanitizer report.  Restated here, statement by statement, because bgtok.hpp is HIP text:
//   placement   the blocks of a feed get dst = carried bytes + the n_dst of the blocks in front; the text workspace has carried + sum(n_dst) + 64
//               bytes; a block writes inside [dst, dst + n_dst) at most (tools/sim/inflate_sim.cc shows that of the decoder); the text ends in
//               front of the first bad block
//   tokens      name offsets and lengths as name_of() gives them: a name ends at white space or at the text's end
//   bg_names    block k, lane t: pack[to[k] + i] = text[off[k] + i], i = t, t + 64, ... < len[k]; to = prefix sums of len on the host; the pack
//               buffer has sum(len) bytes
//   make -C cornetto_amd bgsrc_sim && cornetto_amd/bgsrc_sim [seeds]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static bool is_ws(uint32_t c) { return (c - 9u < 5u) | (c == 32u); }

int main(int argc, char **argv)
{
    const int seeds = argc > 1 ? atoi(argv[1]) : 200;
    long long blocks_placed = 0, names_packed = 0;
    for (int seed = 0; seed < seeds; ++seed) {
        std::mt19937_64 rng(seed);
        // ---- placement
        const int64_t n_pend = (int64_t)(rng() % 3 ? rng() % 5000 : 0);
        const int nb = (int)(rng() % 40);
        std::vector<int32_t> n_dst(nb);
        int64_t n_new = 0;
        for (auto &x : n_dst) {
            const int pick = (int)(rng() % 8);
            x = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 65536 : (int32_t)(rng() % 3000);
            n_new += x;
        }
        const int64_t n = n_pend + n_new;
        uint8_t *text = (uint8_t *)malloc((size_t)n + 64);          // cn_ws(h, WS_BG_TEXT_x, n + 64)
        if (!text) return 2;
        static const char alphabet[] = "ab_1 \t\n09-c";
        for (int64_t i = 0; i < n_pend; ++i) text[i] = (uint8_t)alphabet[rng() % (sizeof(alphabet) - 1)];
        const int bad = nb && rng() % 3 == 0 ? (int)(rng() % nb) : -1;
        int64_t at = n_pend, good_end = n;
        for (int k = 0; k < nb; ++k) {
            const int64_t dst = at;                                   // bgsrc_inflate: k.dst = at; at += k.n_dst
            at += n_dst[k];
            if (k == bad) good_end = dst;
            // the decoder's stores: inside the block's own range, for a bad block some prefix of it
            const int64_t wrote = k == bad ? (int64_t)(rng() % (uint64_t)(n_dst[k] + 1)) : n_dst[k];
            for (int64_t i = 0; i < wrote; ++i) text[dst + i] = (uint8_t)alphabet[rng() % (sizeof(alphabet) - 1)];
            ++blocks_placed;
        }
        if (at != n) { fprintf(stderr, "seed %d: the blocks end at %lld of %lld\n", seed, (long long)at, (long long)n); return 1; }
        const int64_t n_text = bad >= 0 ? good_end : n;               // the text ends in front of the first bad block
        // ---- token starts, then every fourth token as a name (name_of)
        std::vector<uint32_t> off, len;
        int64_t tok = 0;
        for (int64_t p = 0; p < n_text; ++p) {
            if (is_ws(text[p]) || (p > 0 && !is_ws(text[p - 1]))) continue;
            if (tok++ % 4) continue;
            int64_t e = p;
            while (e < n_text && !is_ws(text[e])) ++e;
            off.push_back((uint32_t)p);
            len.push_back((uint32_t)(e - p));
        }
        // ---- bg_names
        std::vector<uint32_t> to(off.size());
        size_t total = 0;
        for (size_t k = 0; k < off.size(); ++k) {
            to[k] = (uint32_t)total;
            total += len[k];
        }
        uint8_t *pack = (uint8_t *)malloc(total ? total : 1);         // the bytes behind the table in WS_BZ_PACK
        if (!pack) return 2;
        for (size_t k = 0; k < off.size(); ++k)
            for (uint32_t t = 0; t < 64; ++t)
                for (uint32_t i = t; i < len[k]; i += 64) pack[to[k] + i] = text[off[k] + i];
        for (size_t k = 0; k < off.size(); ++k) {
            if (memcmp(pack + to[k], text + off[k], len[k]) != 0) { fprintf(stderr, "seed %d: name %zu differs\n", seed, k); return 1; }
            for (uint32_t i = 0; i < len[k]; ++i)
                if (is_ws(pack[to[k] + i])) { fprintf(stderr, "seed %d: white space inside name %zu\n", seed, k); return 1; }
            ++names_packed;
        }
        free(pack);
        free(text);
    }
    printf("bgsrc_sim: %d seeds, %lld blocks placed, %lld names packed: ok\n", seeds, blocks_placed, names_packed);
    return 0;
}
