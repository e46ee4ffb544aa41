// ktrio_sim.cc — the tagged table and the ordered pass of `cornetto trioeval` (cornetto_amd/csrc/kqv.hpp, ktrio.hpp) on the CPU.  The same calls as
// in kt_insert, kt_mark, kt_tile and kt_seam (ktrio.hip) — one tile after the other, inside a tile one thread or lane after the other; the wave
// scan, the wave sum, the ballots and the shuffles are loops over the 64 lanes here — with every contig, the table, the two bitmaps, the tile
// bytes and the counters each in a heap block of exactly its size, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/ktrio_sim.cc -o ktrio_sim
//   ktrio_sim case.bin
// case.bin: "k slots n_batches\n", per parental batch "tag n_contigs\n" (tag 1 pat, 2 mat) and per contig "len\n" + len raw bytes + "\n"; then the
// assembly as one more batch with tag 0.
// stdout: "set <positions> <distinct>" or "overflow"; then per assembly contig "c <kmers> <pat> <mat> <pp> <pm> <mp> <mm>" — which
// tests/test_ktrio_host.py compares with the plain-Python sets of tests/ktrio_cases.py.  Exit 0 and no sanitizer report: the argument for the
// bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cornetto_amd/csrc/ktrio.hpp"

struct Contig {
    uint8_t *seq;
    int64_t len;
};

static bool read_batch(FILE *fp, std::vector<Contig> &b, long long &tag)
{
    long long n;
    if (fscanf(fp, "%lld %lld", &tag, &n) != 2 || fgetc(fp) != '\n') return false;
    for (long long i = 0; i < n; ++i) {
        long long len;
        if (fscanf(fp, "%lld", &len) != 1 || fgetc(fp) != '\n') return false;
        Contig c = {(uint8_t *)malloc((size_t)len), len};   // (exactly its bytes: no padding behind a contig here)
        if (len && fread(c.seq, 1, (size_t)len, fp) != (size_t)len) return false;
        if (fgetc(fp) != '\n') return false;
        b.push_back(c);
    }
    return true;
}

// the tile table of tiles.hpp: first[c] = index of contig c's first tile
static std::vector<int64_t> tile_prefix(const std::vector<Contig> &b)
{
    std::vector<int64_t> first(b.size() + 1, 0);
    for (size_t c = 0; c < b.size(); ++c) first[c + 1] = first[c] + (b[c].len + KQ_TILE - 1) / KQ_TILE;
    return first;
}

int main(int argc, char **argv)
{
    FILE *fp = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    if (!fp) return 2;
    long long k, slots, n_batches;
    if (fscanf(fp, "%lld %lld %lld", &k, &slots, &n_batches) != 3 || fgetc(fp) != '\n' || !kq_k_ok((int)k) || slots < 1) return 2;
    uint64_t *tab = (uint64_t *)malloc((size_t)slots * 8);
    memset(tab, 0xFF, (size_t)slots * 8);
    auto cas = [](uint64_t *p, uint64_t expect, uint64_t val) -> uint64_t {
        const uint64_t old = *p;
        if (old == expect) *p = val;
        return old;
    };
    auto fetch_or = [](uint64_t *p, uint64_t bits) -> uint64_t {
        const uint64_t old = *p;
        *p = old | bits;
        return old;
    };
    bool full = false;
    auto stop = [&full]() { return full; };
    long long n_pos = 0, n_new = 0;
    for (long long bi = 0; bi < n_batches; ++bi) {   // kt_insert, a launch per batch
        std::vector<Contig> b;
        long long tag;
        if (!read_batch(fp, b, tag) || (tag != KT_PAT && tag != KT_MAT)) return 2;
        const std::vector<int64_t> first = tile_prefix(b);
        for (size_t c = 0; c < b.size(); ++c)
            for (int64_t t = first[c]; t < first[c + 1]; ++t)
                for (int tid = 0; tid < KQ_THREADS; ++tid)
                    kq_run(b[c].seq, b[c].len, (t - first[c]) * KQ_TILE, tid, (int)k, [&](int64_t, uint64_t key) {
                        const int res = kq_insert_tag(tab, (uint64_t)slots, key, (uint64_t)tag, cas, fetch_or, stop);
                        n_pos += res != KQ_FULL;
                        n_new += res == KQ_NEW;
                        full |= res == KQ_FULL;
                    });
        for (Contig &c : b) free(c.seq);
    }
    if (full) {
        printf("overflow\n");
        free(tab);
        fclose(fp);
        return 0;
    }
    printf("set %lld %lld\n", n_pos, n_new);

    std::vector<Contig> q;
    long long tag;
    if (!read_batch(fp, q, tag) || tag != 0) return 2;
    fclose(fp);
    const std::vector<int64_t> first = tile_prefix(q);
    const int64_t nt = first[q.size()], nw = nt * KT_WORDS;
    uint64_t *pat = (uint64_t *)calloc((size_t)nw, 8), *mat = (uint64_t *)calloc((size_t)nw, 8);
    uint8_t *tb = (uint8_t *)malloc((size_t)nt);
    int64_t *cnt = (int64_t *)calloc(q.size() * KT_COUNTS, 8);
    std::vector<int32_t> tile_ctg((size_t)nt);
    for (size_t c = 0; c < q.size(); ++c)   // kt_mark
        for (int64_t t = first[c]; t < first[c + 1]; ++t) {
            tile_ctg[(size_t)t] = (int32_t)c;
            for (int tid = 0; tid < KQ_THREADS; ++tid)
                kq_run(q[c].seq, q[c].len, (t - first[c]) * KQ_TILE, tid, (int)k, [&](int64_t pos, uint64_t key) {
                    ++cnt[KT_COUNTS * c + 0];
                    const int tg = kq_lookup_tag(tab, (uint64_t)slots, key);
                    if (tg != KT_PAT && tg != KT_MAT) return;
                    ++cnt[KT_COUNTS * c + tg];
                    int64_t word;
                    uint64_t mask;
                    kq_bit(first[c], pos, word, mask);
                    (tg == KT_PAT ? pat : mat)[word] |= mask;
                });
        }
    for (int64_t t = 0; t < nt; ++t) {   // kt_tile: a wave per tile, a lane per word
        int incl[KT_WORDS];
        for (int l = 0; l < KT_WORDS; ++l) incl[l] = kt_last(pat[t * KT_WORDS + l], mat[t * KT_WORDS + l]);
        for (int d = 1; d < KT_WORDS; d <<= 1)   // the 6 steps of the wave scan: every lane reads lane l - d of the step before
            for (int l = KT_WORDS - 1; l >= d; --l) incl[l] = kt_op(incl[l - d], incl[l]);
        uint64_t pairs = 0;
        int first_type = KT_NONE;
        for (int l = 0; l < KT_WORDS; ++l) {
            const uint64_t p = pat[t * KT_WORDS + l], m = mat[t * KT_WORDS + l];
            pairs += kt_word(p, m, l ? incl[l - 1] : KT_NONE);
            if (first_type == KT_NONE) first_type = kt_first(p, m);   // the lowest lane of the ballot
        }
        tb[t] = kt_tile_byte(first_type, incl[KT_WORDS - 1]);
        for (int i = 0; i < 4; ++i) cnt[KT_COUNTS * tile_ctg[(size_t)t] + 3 + i] += (int64_t)((pairs >> (16 * i)) & 0xFFFF);
    }
    for (int64_t t = 0; t < nt; ++t) {   // kt_seam: a wave per tile, a lane per tile in front
        const int64_t t0 = first[(size_t)tile_ctg[(size_t)t]];
        const int own = kt_byte_first(tb[t]);
        if (own == KT_NONE || t == t0) continue;
        for (int64_t hi = t; hi > t0; hi -= KT_WORDS) {
            int last = KT_NONE;
            for (int l = KT_WORDS - 1; l >= 0; --l) {   // (every lane looks; the lowest lane that found one wins)
                const int v = kt_seam_look(tb, t0, hi, l);
                if (v != KT_NONE) last = v;
            }
            if (last == KT_NONE) continue;
            ++cnt[KT_COUNTS * tile_ctg[(size_t)t] + 3 + kt_pair(last, own)];
            break;
        }
    }
    for (size_t c = 0; c < q.size(); ++c) {
        printf("c");
        for (int i = 0; i < KT_COUNTS; ++i) printf(" %lld", (long long)cnt[KT_COUNTS * c + i]);
        printf("\n");
    }
    free(cnt);
    free(tb);
    free(mat);
    free(pat);
    for (Contig &c : q) free(c.seq);
    free(tab);
    return 0;
}
