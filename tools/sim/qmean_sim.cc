// qmean_sim.cc — the chunk / range / lane-mask arithmetic of `seq -q` (cornetto_amd/csrc/qmean.hpp) on the CPU.  The same statements as in
// qmean_sum (qmean.hip), one wave after the other and inside a wave one lane after the other, over one window and its table of ranges; the
// window (rounded up to the 16 bytes an aligned load may reach: the device has 256 behind it), the starts, the lengths, the sums and the
// 256-entry weight table live in heap blocks of exactly their size, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/qmean_sim.cc -o qmean_sim
//   qmean_sim [--bam] window.bin ranges.txt
// ranges.txt: a line "start len" per range, ascending, not overlapping; --bam: the table of raw BAM qualities in place of the one of printed
// FASTQ characters.  stdout: a line per range, its sum — which tests/test_qmean_host.py compares with the plain-integer sums of
// tests/qmean_cases.py.  Exit 0 and no sanitizer report: the argument for the bounds of the kernel.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cornetto_amd/csrc/qmean.hpp"

int main(int argc, char **argv)
{
    int bam = 0;
    const char *paths[2] = {nullptr, nullptr};
    int n_paths = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--bam")) bam = 1;
        else if (n_paths < 2) paths[n_paths++] = argv[i];
    }
    FILE *fp = n_paths == 2 ? fopen(paths[0], "rb") : nullptr, *fr = n_paths == 2 ? fopen(paths[1], "r") : nullptr;
    if (!fp || !fr) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(fp);
    std::vector<unsigned long long> rs, rl;
    for (unsigned long long s, l; fscanf(fr, "%llu %llu", &s, &l) == 2;) {
        rs.push_back(s);
        rl.push_back(l);
    }
    fclose(fr);
    const int64_t n_text = (int64_t)file.size(), n = (int64_t)rs.size();
    uint8_t *text = (uint8_t *)calloc((size_t)(n_text ? (n_text + 15) / 16 * 16 : 16), 1);
    if (n_text) memcpy(text, file.data(), (size_t)n_text);
    uint32_t *start = (uint32_t *)malloc((size_t)(n ? n : 1) * 4), *len = (uint32_t *)malloc((size_t)(n ? n : 1) * 4);
    uint64_t *sum = (uint64_t *)calloc((size_t)(n ? n : 1), 8);
    uint32_t *tab = (uint32_t *)malloc(256 * 4);
    for (int64_t r = 0; r < n; ++r) {
        if (rs[(size_t)r] + rl[(size_t)r] > (unsigned long long)n_text) return 3;      // (what the callers guarantee: a range lies in the window)
        start[r] = (uint32_t)rs[(size_t)r];
        len[r] = (uint32_t)rl[(size_t)r];
    }
    for (int t = 0; t < 256; ++t) tab[t] = qm_weight(t, bam);
    // qmean_sum: a wave per chunk
    for (int64_t c0 = 0; c0 < n_text; c0 += QM_CHUNK) {
        const int64_t c1 = n_text - c0 < QM_CHUNK ? n_text : c0 + QM_CHUNK;
        int64_t r0 = qm_first(start, len, n, c0);
        if (r0 >= n || (int64_t)start[r0] >= c1) continue;
        for (int lane = 0; lane < QM_LANES; ++lane) {
            const int64_t pos = c0 + (int64_t)lane * 16;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (pos < c1) memcpy(w, text + pos, 16);
            for (int64_t r = r0; r < n; ++r) {
                const int64_t s = (int64_t)start[r];
                if (s >= c1) break;
                const int64_t e = s + (int64_t)len[r];
                if (e <= s || e <= c0) continue;
                int lo, hi;
                qm_span(pos, s, e < c1 ? e : c1, lo, hi);
                sum[r] += qm_lane(w, lo, hi, tab);      // (the wave reduction and its one atomic add)
            }
        }
    }
    for (int64_t r = 0; r < n; ++r) printf("%llu\n", (unsigned long long)sum[r]);
    free(tab);
    free(sum);
    free(len);
    free(start);
    free(text);
    return 0;
}
