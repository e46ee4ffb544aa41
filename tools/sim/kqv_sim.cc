// kqv_sim.cc — the k-mer extraction, the table probes and the run bitmap of `cornetto qv` (cornetto_amd/csrc/kqv.hpp) on the CPU.  The same
// calls as in kq_insert, kq_query, kq_run_count and kq_run_emit (kqv.hip) — one tile after the other, inside a tile one thread after the other:
// kq_run() is the three calls a thread of the kernels makes — with every contig, the table, the bitmap, the per-word counts and the rows each in
// a heap block of exactly its size, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/kqv_sim.cc -o kqv_sim
//   kqv_sim case.bin
// case.bin: "k slots n_batches\n", per truth batch "n_contigs\n" and per contig "len\n" + len raw bytes + "\n"; then the query as one more batch.
// stdout: "set <positions> <distinct>" or "overflow"; then per query contig "c <kmers> <missing>", then per row "r <ctg> <start> <finish>" —
// which tests/test_kqv_host.py compares with the plain-Python set of tests/kqv_cases.py.  Exit 0 and no sanitizer report: the argument for the
// bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cornetto_amd/csrc/kqv.hpp"

struct Contig {
    uint8_t *seq;
    int64_t len;
};

static bool read_batch(FILE *fp, std::vector<Contig> &b)
{
    long long n;
    if (fscanf(fp, "%lld", &n) != 1 || fgetc(fp) != '\n') return false;
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
    bool full = false;
    auto stop = [&full]() { return full; };
    long long n_pos = 0, n_new = 0;
    for (long long bi = 0; bi < n_batches; ++bi) {   // kq_insert, a launch per batch
        std::vector<Contig> b;
        if (!read_batch(fp, b)) return 2;
        const std::vector<int64_t> first = tile_prefix(b);
        for (size_t c = 0; c < b.size(); ++c)
            for (int64_t t = first[c]; t < first[c + 1]; ++t)
                for (int tid = 0; tid < KQ_THREADS; ++tid)
                    kq_run(b[c].seq, b[c].len, (t - first[c]) * KQ_TILE, tid, (int)k, [&](int64_t, uint64_t key) {
                        const int res = kq_insert(tab, (uint64_t)slots, key, cas, stop);
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
    if (!read_batch(fp, q)) return 2;
    fclose(fp);
    const std::vector<int64_t> first = tile_prefix(q);
    const int64_t nt = first[q.size()], nw = nt * (KQ_TILE / 64);
    uint64_t *bits = (uint64_t *)calloc((size_t)nw, 8);
    std::vector<int32_t> tile_ctg((size_t)nt), tile_first((size_t)nt);
    for (size_t c = 0; c < q.size(); ++c) {   // kq_query
        long long kmers = 0, missing = 0;
        for (int64_t t = first[c]; t < first[c + 1]; ++t) {
            tile_ctg[(size_t)t] = (int32_t)c;
            tile_first[(size_t)t] = (int32_t)((t - first[c]) * KQ_TILE);
            for (int tid = 0; tid < KQ_THREADS; ++tid)
                kq_run(q[c].seq, q[c].len, (t - first[c]) * KQ_TILE, tid, (int)k, [&](int64_t pos, uint64_t key) {
                    ++kmers;
                    if (kq_lookup(tab, (uint64_t)slots, key)) return;
                    ++missing;
                    int64_t word;
                    uint64_t mask;
                    kq_bit(first[c], pos, word, mask);
                    bits[word] |= mask;
                });
        }
        printf("c %lld %lld\n", kmers, missing);
    }
    // kq_run_count, the scan, kq_run_emit
    uint32_t *cnt = (uint32_t *)malloc((size_t)nw * 4), *rank = (uint32_t *)malloc((size_t)nw * 4);
    uint32_t total = 0;
    for (int64_t w = 0; w < nw; ++w) {
        cnt[w] = (uint32_t)__builtin_popcountll(kq_starts(bits[w], w ? bits[w - 1] >> 63 : 0));
        rank[w] = total;
        total += cnt[w];
    }
    cornetto_ivl_t *rows = (cornetto_ivl_t *)malloc((size_t)total * sizeof(cornetto_ivl_t));
    for (int64_t w = 0; w < nw; ++w) {
        const uint64_t v = bits[w];
        if (!v) continue;
        const uint64_t prev = w ? bits[w - 1] >> 63 : 0, next = w + 1 < nw ? bits[w + 1] : 0;
        const int64_t t = w / (KQ_TILE / 64);
        const int32_t p0 = tile_first[(size_t)t] + (int32_t)(w % (KQ_TILE / 64)) * 64;
        uint32_t r = rank[w];
        for (uint64_t m = kq_starts(v, prev); m; m &= m - 1, ++r) {
            rows[r].ctg = tile_ctg[(size_t)t];
            rows[r].start = p0 + __builtin_ctzll(m);
        }
        r = kq_end_rank(rank[w], v, prev);
        for (uint64_t m = kq_ends(v, next); m; m &= m - 1, ++r) rows[r].finish = p0 + __builtin_ctzll(m) + (int32_t)k;
    }
    // the merge with distance 0 (ivlmerge.hpp's sequential rule): an interval that starts at or before the largest finish so far in its contig
    for (uint32_t i = 0; i < total;) {
        cornetto_ivl_t cur = rows[i++];
        for (; i < total && rows[i].ctg == cur.ctg && rows[i].start <= cur.finish; ++i)
            if (rows[i].finish > cur.finish) cur.finish = rows[i].finish;
        printf("r %d %d %d\n", cur.ctg, cur.start, cur.finish);
    }
    free(rows);
    free(rank);
    free(cnt);
    free(bits);
    for (Contig &c : q) free(c.seq);
    free(tab);
    return 0;
}
