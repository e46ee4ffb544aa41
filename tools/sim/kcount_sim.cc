// kcount_sim.cc — the counted k-mer table of `cornetto qv -r` / `cornetto trioeval --pat-reads --mat-reads` (cornetto_amd/csrc/kqv.hpp) on the CPU.
// The same calls as in kq_count, kq_hist and kq_seal (kcount.hip) and in the probes of kq_query (kqv.hip) and kt_mark (ktrio.hip) — one workgroup
// after the other, inside it one thread after the other, the lanes behind the last run included — with every record, the prefix, the table, the
// counts and the histogram each in a heap block of exactly its size, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/kcount_sim.cc -o kcount_sim
//   kcount_sim case.bin
// case.bin: "k slots channels n_batches\n"; per batch of reads "channel\n", "n_records\n" and per record "len\n" + len raw bytes + "\n"; then
// "m0 m1\n" (the thresholds) and the query as one more batch without a channel line.
// stdout: "set <positions> <distinct>" or "overflow"; per channel and non-zero bin "h <channel> <bin> <keys>"; "solid <s0> [<s1>]"; then per query
// contig, one channel: "c <kmers> <missing>"; two channels: "t <kmers> <pat> <mat> <pp> <pm> <mp> <mm>" (the lookups of the tagged table in
// position order, paired as the rule pairs them) — which tests/test_kcount_host.py compares with the Counter of tests/kcount_cases.py.
// Exit 0 and no sanitizer report: the argument for the bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    long long k, slots, channels, n_batches;
    if (fscanf(fp, "%lld %lld %lld %lld", &k, &slots, &channels, &n_batches) != 4 || fgetc(fp) != '\n' || !kq_k_ok((int)k) || slots < 1 || channels < 1 || channels > 2)
        return 2;
    uint64_t *tab = (uint64_t *)malloc((size_t)slots * 8);
    memset(tab, 0xFF, (size_t)slots * 8);
    uint32_t *cnt = (uint32_t *)calloc((size_t)(slots * channels), 4);
    auto cas = [](uint64_t *p, uint64_t expect, uint64_t val) -> uint64_t {
        const uint64_t old = *p;
        if (old == expect) *p = val;
        return old;
    };
    bool full = false;
    auto stop = [&full]() { return full; };
    auto load = [](uint32_t *p) -> uint32_t { return *p; };
    auto add = [](uint32_t *p) { ++*p; };
    long long n_pos = 0, n_new = 0;
    for (long long bi = 0; bi < n_batches; ++bi) {   // kq_count, a launch per batch
        long long ch;
        if (fscanf(fp, "%lld", &ch) != 1 || fgetc(fp) != '\n' || ch < 0 || ch >= channels) return 2;
        std::vector<Rec> b;
        if (!read_batch(fp, b)) return 2;
        const int n = (int)b.size();
        int64_t *first = (int64_t *)malloc(((size_t)n + 1) * 8);   // tiles.hpp's prefix, of the runs of the records
        first[0] = 0;
        for (int c = 0; c < n; ++c) first[c + 1] = first[c] + kq_runs_of(b[(size_t)c].len);
        const int64_t nr = first[n], nb = (nr + KQ_THREADS - 1) / KQ_THREADS;
        uint32_t *ch_cnt = cnt + ch * slots;
        for (int64_t g = 0; g < nb * KQ_THREADS; ++g) {   // every thread of every workgroup
            const uint8_t *seq = nullptr;
            int64_t b0 = 0, b1 = 0;
            if (g < nr) {
                const int c = kq_record_of(first, n, g);
                seq = b[(size_t)c].seq;
                kq_deal(g - first[c], b[(size_t)c].len, b0, b1);
                if (b0 >= b1) return 3;   // every dealt run owns a base
            }
            KqRoll s = {0, 0, 0};
            if (b0 < b1) s = kq_lead(seq, b0, (int)k);
            for (int r = 0; r < KQ_RUN; ++r) {
                int64_t pos;
                uint64_t key, at = 0;
                const bool has = kq_step(seq, b0, b1, r, s, (int)k, pos, key);
                const int res = has ? kq_insert_at(tab, (uint64_t)slots, key, cas, stop, at) : KQ_PRESENT;
                if (has && res != KQ_FULL) kq_bump(ch_cnt + at, load, add);
                n_pos += has && res != KQ_FULL;
                n_new += res == KQ_NEW;
                full |= res == KQ_FULL;
            }
        }
        free(first);
        for (Rec &c : b) free(c.seq);
    }
    if (full) {
        printf("overflow\n");
        free(cnt);
        free(tab);
        fclose(fp);
        return 0;
    }
    printf("set %lld %lld\n", n_pos, n_new);

    for (long long ch = 0; ch < channels; ++ch) {   // kq_hist
        unsigned long long *hist = (unsigned long long *)calloc(KQ_BINS, 8);
        for (long long i = 0; i < slots; ++i) {
            const uint32_t c = cnt[ch * slots + i];
            if (c) ++hist[kq_hist_bin(c)];
        }
        for (int i = 0; i < KQ_BINS; ++i)
            if (hist[i]) printf("h %lld %d %llu\n", ch, i, hist[i]);
        free(hist);
    }

    long long m[2] = {1, 1}, solid[2] = {0, 0};
    if (fscanf(fp, "%lld %lld", &m[0], &m[1]) != 2 || fgetc(fp) != '\n' || m[0] < 1 || m[1] < 1) return 2;
    for (long long i = 0; i < slots; ++i) {   // kq_seal
        const uint64_t key = tab[i];
        if (key == KQ_EMPTY) continue;
        const bool s0 = kq_count_of(cnt[i]) >= (uint32_t)m[0];
        const bool s1 = channels == 2 && kq_count_of(cnt[slots + i]) >= (uint32_t)m[1];
        tab[i] = kq_seal_word(key, (int)channels, (s0 ? 1 : 0) | (s1 ? 2 : 0));
        solid[0] += s0;
        solid[1] += s1;
    }
    free(cnt);   // (as the seal frees the counts: nothing behind it reads them)
    if (channels == 1) printf("solid %lld\n", solid[0]);
    else printf("solid %lld %lld\n", solid[0], solid[1]);

    std::vector<Rec> q;
    if (!read_batch(fp, q)) return 2;
    fclose(fp);
    for (Rec &c : q) {   // kq_query / kt_mark: a workgroup per tile, the probes with plain loads
        long long t[7] = {0, 0, 0, 0, 0, 0, 0}, missing = 0;
        int prev = 0;
        for (int64_t first = 0; first < c.len; first += KQ_TILE)
            for (int tid = 0; tid < KQ_THREADS; ++tid)
                kq_run(c.seq, c.len, first, tid, (int)k, [&](int64_t, uint64_t key) {
                    ++t[0];
                    if (channels == 1) {
                        missing += !kq_lookup(tab, (uint64_t)slots, key);
                        return;
                    }
                    const int tag = kq_lookup_tag(tab, (uint64_t)slots, key);
                    if (tag != 1 && tag != 2) return;
                    ++t[tag];
                    if (prev) ++t[3 + (prev - 1) * 2 + (tag - 1)];
                    prev = tag;
                });
        if (channels == 1) printf("c %lld %lld\n", t[0], missing);
        else printf("t %lld %lld %lld %lld %lld %lld %lld\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
        free(c.seq);
    }
    free(tab);
    return 0;
}
