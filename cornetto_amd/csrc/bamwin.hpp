// bamwin.hpp — the window of inflated BAM that bam.hip (cornetto_bamdepth_*) and bamfq.hip (cornetto_bamfq_*) both work on: the blocks of a
// feed get their places behind the tail the last window left (win_place), are inflated there (win_inflate: cornetto_text_inflate; a bad block
// cuts the window in front of it), the record chain is followed by one wave (win_frame: bam_frame) and the bytes behind the last whole
// record are moved to the front (win_carry).  The two stages differ in what they do with the framed records between win_frame and win_carry.
#pragma once
#include "bam.hpp"
#include "common.hpp"

namespace cnbw {
namespace {   // internal linkage: every translation unit that includes this gets its own copy

// words of the small device block; a stage keeps its own counters from BW_OWN on
enum { BW_NREC = 0, BW_END = 1, BW_FERR = 2, BW_FERR_A = 3, BW_ERR = 4, BW_OWN = 5, BW_WORDS = 16 };

__global__ void __launch_bounds__(64) bam_frame(const uint8_t *__restrict__ text, int64_t at, int64_t n, uint32_t *__restrict__ off, int64_t cap, unsigned long long *sm)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t end;
    int32_t err, a;
    const int64_t k = cnb_frame(text, at, n, off, cap, &end, &err, &a);
    sm[BW_NREC] = (unsigned long long)k;
    sm[BW_END] = (unsigned long long)end;
    sm[BW_FERR] = (unsigned long long)err;
    sm[BW_FERR_A] = (unsigned long long)(long long)a;
}

struct Win {
    int64_t window = 0;                // bytes of inflated BAM held at once
    cornetto_text_t *win = nullptr;    // the window
    uint8_t *d_tail = nullptr;         // staging of a tail that overlaps its new place
    uint32_t *d_recoff = nullptr;
    int64_t rec_cap = 0;
    unsigned long long *d_sm = nullptr;
    int64_t carry = 0, skip_left = 0, text_off = 0, n_rec = 0, n_blocks = 0;
};

void win_close(cornetto_accel_t *h, Win &w)
{
    if (w.win) cornetto_text_free(h, w.win);
    void *blocks[] = {w.d_tail, w.d_recoff, w.d_sm};
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    w.win = nullptr;
    w.d_tail = nullptr;
    w.d_recoff = nullptr;
    w.d_sm = nullptr;
}

// CORNETTO_OK, or the status of cornetto_text_open(), or CORNETTO_E_NOMEM (nothing is said: the caller names its arrays)
int win_open(cornetto_accel_t *h, Win &w, int64_t window)
{
    w.window = window;
    w.rec_cap = window / 36 + 2;
    CN_TRY(cornetto_text_open(h, window, &w.win));
    const bool ok = hipMalloc((void **)&w.d_tail, (size_t)window) == hipSuccess && hipMalloc((void **)&w.d_recoff, (size_t)w.rec_cap * 4) == hipSuccess &&
                    hipMalloc((void **)&w.d_sm, BW_WORDS * 8) == hipSuccess;
    return ok ? CORNETTO_OK : CORNETTO_E_NOMEM;
}

// the leading blocks of blocks[0 .. n) that fit behind the carried tail, with their places -> grp; *fill: the window's bytes with them
int64_t win_place(const Win &w, const cornetto_bgzf_block_t *blocks, int64_t n, std::vector<cornetto_bgzf_block_t> &grp, int64_t *fill)
{
    grp.clear();
    int64_t f = w.carry, j = 0;
    while (j < n && f + blocks[j].n_dst <= w.window) {
        cornetto_bgzf_block_t x = blocks[j];
        x.dst = f;
        f += x.n_dst;
        grp.push_back(x);
        ++j;
    }
    *fill = f;
    return j;
}

// the records of window bytes [0, n_text): the bytes to skip, then the chain -> *n records (their offsets in d_recoff), *end, the chain's error
int win_frame(cornetto_accel_t *h, Win &w, const char *who, int64_t n_text, unsigned long long *p_sm, int64_t *n, int64_t *end, int *ferr, int64_t *ferr_a)
{
    const int64_t start = std::min(w.skip_left, n_text);      // (bytes are skipped only while nothing is carried)
    w.skip_left -= start;
    CN_HIP(h, hipMemsetAsync(w.d_sm, 0, BW_WORDS * 8, h->stream));
    CN_HIP(h, hipMemsetAsync(w.d_sm + BW_ERR, 0xFF, 8, h->stream));
    CN_LAUNCH(h, "bam_frame", bam_frame<<<dim3(1), dim3(64), 0, h->stream>>>(w.win->d, start, n_text, w.d_recoff, w.rec_cap, w.d_sm));
    CN_HIP(h, hipMemcpyAsync(p_sm, w.d_sm, 32, hipMemcpyDeviceToHost, h->stream));
    CN_HIP(h, hipStreamSynchronize(h->stream));
    *n = (int64_t)p_sm[BW_NREC];
    *end = (int64_t)p_sm[BW_END];
    *ferr = (int)p_sm[BW_FERR];
    *ferr_a = (int64_t)p_sm[BW_FERR_A];
    if (*n < 0 || *n > w.rec_cap || *end < start || *end > n_text) return cn_fail(h, CORNETTO_E_HIP, "%s: the record chain left its window", who);
    return CORNETTO_OK;
}

// the bytes [end, n_text) of the window open the next one
int win_carry(cornetto_accel_t *h, Win &w, int64_t n_text, int64_t end)
{
    const int64_t carry = n_text - end;
    if (carry > 0 && end > 0) {
        if (carry <= end) {
            CN_HIP(h, hipMemcpyAsync(w.win->d, w.win->d + end, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
        } else {
            CN_HIP(h, hipMemcpyAsync(w.d_tail, w.win->d + end, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
            CN_HIP(h, hipMemcpyAsync(w.win->d, w.d_tail, (size_t)carry, hipMemcpyDeviceToDevice, h->stream));
        }
        CN_HIP(h, hipStreamSynchronize(h->stream));
    }
    w.carry = carry;
    w.text_off += end;
    return CORNETTO_OK;
}

}  // namespace
}  // namespace cnbw
