// fqseq_sim.cc — the framing, the size pass and the text kernel of `seq --fastq` (cornetto_amd/csrc/fqrec.hpp, fqseq.hpp) on the CPU.  The
// same statements as in fq_records / fqseq_size / fqseq_text, one thread of control after the other, over the windows of fqseq.hip's feed; the
// window (with the 256 bytes the device allocates behind it), the newline, record, size and offset tables and the bytes of every get live in
// heap blocks of exactly their size, so that the host sanitizers see every byte read or written outside them:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sim/fqseq_sim.cc -o fqseq_sim
//   fqseq_sim [--window W] [--range R] [--min-len N] text.fq
// The text is taken through windows of W bytes behind the tail the last window left (the whole text by default), and every window's text is
// fetched as the gets of the device fetch it: a first range of 7 bytes, then ranges of R bytes (the whole text by default), so that `at` is
// no multiple of 16, each cut into the kernel's tiles and 16-byte chunks.  stdout: the text; stderr: one line
//   rest plain total_reads total_bases kept_reads kept_bases
// which tests/test_fqseq_host.py compares with the oracle's.  Exit 0 and no sanitizer report: the argument for the bounds of the kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cornetto_amd/csrc/fqseq.hpp"

static const int64_t TILE = CORNETTO_FQSEQ_TILE;

// bytes [at, at + n) of the window's text, as fqseq_text writes them into a slab of n bytes rounded up to 16
static void get(const FxArgs &W, int64_t at, int64_t n, std::vector<uint8_t> &out)
{
    uint8_t *dst = (uint8_t *)malloc((size_t)((n + 15) / 16 * 16));
    FxArgs A = W;
    A.at = at;
    A.nbytes = n;
    A.dst = dst;
    for (int64_t tile = 0; tile < n; tile += TILE) {
        const int64_t t_end = n - tile < TILE ? n - tile : TILE;
        const int64_t r0 = fx_find(A.out, 0, A.n - 1, A.at + tile);
        const int64_t r1 = fx_find(A.out, r0, A.n - 1, A.at + tile + t_end - 1);
        for (int64_t rel = tile; rel < tile + t_end; rel += 16) {
            const int m = (int)(n - rel < 16 ? n - rel : 16);
            const Fx16 v = fx_chunk(A, r0, r1, A.at + rel, m);
            memcpy(dst + rel, v.w, 16);
        }
    }
    out.insert(out.end(), dst, dst + n);
    free(dst);
}

int main(int argc, char **argv)
{
    int64_t window = 0, range = 0;
    int32_t min_len = 0;
    const char *path = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--window") && i + 1 < argc) window = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--range") && i + 1 < argc) range = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-len") && i + 1 < argc) min_len = atoi(argv[++i]);
        else path = argv[i];
    }
    FILE *fp = path ? fopen(path, "rb") : nullptr;
    if (!fp) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(fp);
    if (window <= 0) window = (int64_t)file.size() > 0 ? (int64_t)file.size() : 1;
    uint8_t *win = (uint8_t *)calloc((size_t)window + 256, 1);          // (what the device allocates)
    std::vector<uint8_t> text;
    long long stats[4] = {0, 0, 0, 0};
    int64_t carry = 0, text_off = 0, fed = 0, rest = 0;
    bool stopped = false;
    for (bool first = true; !stopped && (fed < (int64_t)file.size() || first); first = false) {
        const int64_t got = std::min<int64_t>((int64_t)file.size() - fed, window - carry);
        if (got == 0 && fed < (int64_t)file.size()) {          // a record larger than the window: CORNETTO_E_NOMEM on the device
            stopped = true;
            break;
        }
        if (got > 0) memcpy(win + carry, file.data() + fed, (size_t)got);
        fed += got;
        const int64_t n = carry + got;
        const bool final = fed == (int64_t)file.size();
        // the newline index, in a block of its own
        int64_t n_nl = 0;
        for (int64_t i = 0; i < n; ++i) n_nl += win[i] == '\n';
        uint32_t *nl = (uint32_t *)malloc((size_t)(n_nl ? n_nl : 1) * 4);
        for (int64_t i = 0, k = 0; i < n; ++i)
            if (win[i] == '\n') nl[k++] = (uint32_t)i;
        const int64_t n_lines = n_nl + (final && n > 0 && win[n - 1] != '\n' ? 1 : 0), n_rec = n_lines / 4;
        cornetto_fqrec_t *recs = (cornetto_fqrec_t *)malloc((size_t)(n_rec ? n_rec : 1) * sizeof(cornetto_fqrec_t));
        uint32_t *ends = (uint32_t *)malloc((size_t)(n_rec ? n_rec : 1) * 4);
        FqArgs F{win, n, nl, n_nl, n_rec, min_len, recs, nullptr, ends};
        int64_t n_use = n_rec;
        for (int64_t r = 0; r < n_rec; ++r)
            if (!fq_frame(F, r, recs[r], ends[r]) && r < n_use) n_use = r;
        for (int64_t i = 0; i < n; ++i)          // fqseq_zero / fqseq_fold
            if (win[i] == 0) {
                for (int64_t r = 0; r < n_use; ++r)
                    if (ends[r] > (uint32_t)i) {
                        n_use = r;
                        break;
                    }
                break;
            }
        if (n_use < n_rec) stopped = true;
        const int64_t end = n_use ? ends[n_use - 1] : 0;
        if (final && end < n) stopped = true;
        uint32_t *out = (uint32_t *)malloc((size_t)(n_use + 1) * 4);
        uint32_t total = 0;
        for (int64_t r = 0; r < n_use; ++r) {
            out[r] = total;
            total += fx_size(recs[r]);
            stats[0] += 1;
            stats[1] += recs[r].len;
            if (recs[r].keep) {
                stats[2] += 1;
                stats[3] += recs[r].len;
            }
        }
        out[n_use] = total;
        FxArgs W{win, recs, out, n_use, 0, 0, nullptr};
        for (int64_t at = 0; at < (int64_t)total;) {
            const int64_t k = std::min<int64_t>((int64_t)total - at, at == 0 ? 7 : (range > 0 ? range : (int64_t)total));
            get(W, at, k, text);
            at += k;
        }
        free(out);
        free(ends);
        free(recs);
        free(nl);
        memmove(win, win + end, (size_t)(n - end));
        carry = n - end;
        text_off += end;
        rest = text_off;
    }
    free(win);
    if (!text.empty()) fwrite(text.data(), 1, text.size(), stdout);
    fprintf(stderr, "%lld %d %lld %lld %lld %lld\n", (long long)rest, stopped ? 0 : 1, stats[0], stats[1], stats[2], stats[3]);
    return 0;
}
