// kspec_sim.cc — the copies and the copy-number spectrum of `cornetto qv -r --completeness / --spectra-cn` (cornetto_amd/csrc/kqv.hpp) on the CPU.
// The same calls as in kq_count, kq_copies, kq_spectrum, kq_hist and kq_seal (kcount.hip) — one workgroup after the other, inside it one thread
// after the other, the lanes behind the last run and the last slot included — with every record, the prefix, the table, the counts, the packed
// copies, the workgroup's cells and the spectrum each in a heap block of exactly its size, so that the host sanitizers see every byte read or
// written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/kspec_sim.cc -o kspec_sim
//   kspec_sim case.bin
// case.bin: "k slots n_read_batches\n"; per batch "n_records\n" and per record "len\n" + len raw bytes + "\n"; "n_m\n" and the thresholds, one a
// line; "n_assemblies\n"; per assembly "n_batches\n" and its batches.  The copies are cleared between two assemblies.
// stdout: "set <positions> <distinct>" after the reads; per assembly "asm <i>", per non-zero cell "s <a> <c> <keys>", per threshold
// "t <m> <solid> <found>"; "overflow" and the end where the table has no room; behind the last assembly "set <positions> <distinct>" again, per
// non-zero bin "h <bin> <keys>", and "solid <n>" of the seal with the first threshold — which tests/test_kspec_host.py compares with the Counters of
// tests/kspec_cases.py; "lost <n>": the compare-and-swaps of kq_copy_bump() that failed, because every third load of a word is an old one.
// Exit 0 and no sanitizer report: the argument for the bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "../../cornetto_amd/csrc/kqv.hpp"

struct Rec {
    uint8_t *seq;
    int64_t len;
};

static bool read_batch(FILE *fp, std::vector<Rec> &b)
{
    long long n;
    if (fscanf(fp, "%lld", &n) != 1 || fgetc(fp) != '\n') return false;
    for (long long i = 0; i < n; ++i) {
        long long len;
        if (fscanf(fp, "%lld", &len) != 1 || fgetc(fp) != '\n') return false;
        Rec c = {(uint8_t *)malloc((size_t)len), len};   // (exactly its bytes: no padding behind a record here)
        if (len && fread(c.seq, 1, (size_t)len, fp) != (size_t)len) return false;
        if (fgetc(fp) != '\n') return false;
        b.push_back(c);
    }
    return true;
}

int main(int argc, char **argv)
{
    FILE *fp = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    if (!fp) return 2;
    long long k, slots, n_batches;
    if (fscanf(fp, "%lld %lld %lld", &k, &slots, &n_batches) != 3 || fgetc(fp) != '\n' || !kq_k_ok((int)k) || slots < 1) return 2;
    uint64_t *tab = (uint64_t *)malloc((size_t)slots * 8);
    memset(tab, 0xFF, (size_t)slots * 8);
    uint32_t *cnt = (uint32_t *)calloc((size_t)slots, 4);
    const uint64_t cop_words = kq_copy_words((uint64_t)slots);
    uint32_t *cop = (uint32_t *)calloc((size_t)cop_words, 4);
    auto cas = [](uint64_t *p, uint64_t expect, uint64_t val) -> uint64_t {
        const uint64_t old = *p;
        if (old == expect) *p = val;
        return old;
    };
    bool full = false;
    auto stop = [&full]() { return full; };
    auto load = [](uint32_t *p) -> uint32_t { return *p; };
    auto add = [](uint32_t *p) { ++*p; };
    // the relaxed load of kq_copy_bump() may be old: every third one returns what the word held in front of the last successful swap on it (bytes
    // only grow between two clears, so that is a value the word did hold).  The swap that follows then loses for real — an occurrence has gone in
    // since the value was read — takes the word it is handed and repeats, or leaves if its byte has reached the top meanwhile
    unsigned long long n_load = 0, n_lost = 0;
    std::unordered_map<uint32_t *, uint32_t> before;
    auto load32 = [&](uint32_t *p) -> uint32_t {
        auto it = before.find(p);
        return ++n_load % 3 == 0 && it != before.end() ? it->second : *p;
    };
    auto cas32 = [&](uint32_t *p, uint32_t expect, uint32_t val) -> uint32_t {
        const uint32_t old = *p;
        if (old == expect) {
            before[p] = old;
            *p = val;
        } else ++n_lost;
        return old;
    };
    long long n_pos = 0, n_new = 0;
    for (long long bi = 0; bi < n_batches; ++bi) {   // kq_count, a launch per batch
        std::vector<Rec> b;
        if (!read_batch(fp, b)) return 2;
        const int n = (int)b.size();
        int64_t *first = (int64_t *)malloc(((size_t)n + 1) * 8);
        first[0] = 0;
        for (int c = 0; c < n; ++c) first[c + 1] = first[c] + kq_runs_of(b[(size_t)c].len);
        const int64_t nr = first[n], nb = (nr + KQ_THREADS - 1) / KQ_THREADS;
        for (int64_t g = 0; g < nb * KQ_THREADS; ++g) {
            const uint8_t *seq = nullptr;
            int64_t b0 = 0, b1 = 0;
            if (g < nr) {
                const int c = kq_record_of(first, n, g);
                seq = b[(size_t)c].seq;
                kq_deal(g - first[c], b[(size_t)c].len, b0, b1);
            }
            KqRoll s = {0, 0, 0};
            if (b0 < b1) s = kq_lead(seq, b0, (int)k);
            for (int r = 0; r < KQ_RUN; ++r) {
                int64_t pos;
                uint64_t key, at = 0;
                const bool has = kq_step(seq, b0, b1, r, s, (int)k, pos, key);
                const int res = has ? kq_insert_at(tab, (uint64_t)slots, key, cas, stop, at) : KQ_PRESENT;
                if (has && res != KQ_FULL) kq_bump(cnt + at, load, add);
                n_pos += has && res != KQ_FULL;
                n_new += res == KQ_NEW;
                full |= res == KQ_FULL;
            }
        }
        free(first);
        for (Rec &c : b) free(c.seq);
    }
    if (full) {
        printf("overflow\n");   // (a dead set takes no more calls)
        free(cop);
        free(cnt);
        free(tab);
        fclose(fp);
        return 0;
    }
    printf("set %lld %lld\n", n_pos, n_new);

    long long n_m, n_asm;
    std::vector<long long> ms;
    if (fscanf(fp, "%lld", &n_m) != 1 || fgetc(fp) != '\n' || n_m < 1) return 2;
    for (long long i = 0; i < n_m; ++i) {
        long long m;
        if (fscanf(fp, "%lld", &m) != 1 || fgetc(fp) != '\n' || m < 1 || m > (long long)KQ_CAP) return 2;
        ms.push_back(m);
    }
    if (fscanf(fp, "%lld", &n_asm) != 1 || fgetc(fp) != '\n') return 2;
    for (long long ai = 0; ai < n_asm; ++ai) {
        if (fscanf(fp, "%lld", &n_batches) != 1 || fgetc(fp) != '\n') return 2;
        for (long long bi = 0; bi < n_batches; ++bi) {   // kq_copies, a launch per batch: a workgroup per tile, a thread a run
            std::vector<Rec> b;
            if (!read_batch(fp, b)) return 2;
            for (Rec &c : b) {
                for (int64_t first = 0; first < c.len; first += KQ_TILE)
                    for (int tid = 0; tid < KQ_THREADS; ++tid) {
                        int64_t b0, b1;
                        kq_bounds(first, tid, c.len, b0, b1);
                        KqRoll s = {0, 0, 0};
                        if (b0 < b1) s = kq_lead(c.seq, b0, (int)k);
                        for (int r = 0; r < KQ_RUN; ++r) {
                            int64_t pos;
                            uint64_t key, at = 0;
                            if (!kq_step(c.seq, b0, b1, r, s, (int)k, pos, key)) continue;
                            if (kq_insert_at(tab, (uint64_t)slots, key, cas, stop, at) == KQ_FULL) full = true;
                            else {
                                if (kq_copy_word(at) >= cop_words) return 3;
                                kq_copy_bump(cop + kq_copy_word(at), kq_copy_shift(at), load32, cas32);
                            }
                        }
                    }
                free(c.seq);
            }
        }
        if (full) {
            printf("overflow\n");
            free(cop);
            free(cnt);
            free(tab);
            fclose(fp);
            return 0;
        }
        printf("asm %lld\n", ai);
        for (long long m : ms) {   // kq_spectrum, a launch per threshold: 256 lanes a round, the rounds of a workgroup a stride of blocks apart
            const size_t N = (size_t)KQ_CN_BINS * KQ_BINS;
            unsigned long long *out = (unsigned long long *)calloc(N + 2, 8);
            const uint64_t want = ((uint64_t)slots + 255) / 256, nb = want < 3 ? want : 3;
            for (uint64_t blk = 0; blk < nb; ++blk) {
                uint32_t *cells = (uint32_t *)calloc(N, 4);
                unsigned long long n_solid = 0, n_found = 0;
                for (uint64_t base = blk * 256; base < (uint64_t)slots; base += nb * 256)
                    for (uint64_t tid = 0; tid < 256; ++tid) {
                        const uint64_t i = base + tid;
                        uint32_t c = 0, a = 0;
                        if (i < (uint64_t)slots) {
                            c = cnt[i];
                            a = kq_copy_of(cop[kq_copy_word(i)], i);
                        }
                        if (c | a) ++cells[kq_spec_cell(a, c)];
                        const bool solid = c != 0 && kq_count_of(c) >= (uint32_t)m;
                        n_solid += solid;
                        n_found += solid && a != 0;
                    }
                for (size_t i = 0; i < N; ++i)
                    if (cells[i]) out[i] += cells[i];
                out[N] += n_solid;
                out[N + 1] += n_found;
                free(cells);
            }
            if (m == ms[0])
                for (size_t i = 0; i < N; ++i)
                    if (out[i]) printf("s %d %d %llu\n", (int)(i / KQ_BINS), (int)(i % KQ_BINS), out[i]);
            printf("t %lld %llu %llu\n", m, out[N], out[N + 1]);
            free(out);
        }
        memset(cop, 0, (size_t)cop_words * 4);   // kset_copies_clear
        before.clear();
    }
    fclose(fp);

    printf("set %lld %lld\n", n_pos, n_new);   // (the copies have moved neither)
    unsigned long long *hist = (unsigned long long *)calloc(KQ_BINS, 8);   // kq_hist
    for (long long i = 0; i < slots; ++i)
        if (cnt[i]) ++hist[kq_hist_bin(cnt[i])];
    for (int i = 0; i < KQ_BINS; ++i)
        if (hist[i]) printf("h %d %llu\n", i, hist[i]);
    free(hist);
    long long solid = 0;
    for (long long i = 0; i < slots; ++i) {   // kq_seal: an assembly-only key becomes the tombstone
        const uint64_t key = tab[i];
        if (key == KQ_EMPTY) continue;
        const bool s0 = kq_count_of(cnt[i]) >= (uint32_t)ms[0];
        tab[i] = kq_seal_word(key, 1, s0 ? 1 : 0);
        if (!cnt[i] && tab[i] != KQ_TOMB) return 3;
        solid += s0;
    }
    printf("solid %lld\n", solid);
    printf("lost %llu\n", n_lost);
    free(cop);
    free(cnt);
    free(tab);
    return 0;
}
