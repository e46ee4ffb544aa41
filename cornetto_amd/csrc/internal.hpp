// internal.hpp — pieces of cov.hip / telo.hip that step.hip (cornetto_panel_step) puts together: the same kernels and host
// logic as the public entry points, without their timing brackets and — the "spec" pairs — without their synchronisation.
// Not part of the C ABI.
#pragma once
#include "common.hpp"

// cornetto_cov_prepare() without the timing bracket (synchronises: the sums are on the host when it returns)
int cn_cov_prepare_impl(cornetto_accel_t *h, cornetto_cov_t *c, int32_t w, int32_t inc, uint64_t sums[3]);

// A packed selection (cornetto_cov_select_packed) queued WITHOUT its synchronisation: the result copy is sized by the count the last
// selection with the same parameters gave (cornetto_cov::cw_est_*), the count is checked afterwards.  cn_cov_spec_queue() leaves
// `queued` false when there is no such count (the caller takes cornetto_cov_select_packed()); cn_cov_spec_finish(), called after the
// handle's stream has been synchronised, returns 1 when the count outgrew the copy (nothing is returned: take the exact call), else
// CORNETTO_OK with the results, or an error.
struct CnCovSpec {
    bool queued = false;
    cornetto_regpk_t *o = nullptr;
    size_t n_copy = 0, cap = 0;
    unsigned long long *p_cnt = nullptr;   // pinned, 8 bytes, the caller's
    uint32_t *p_cf = nullptr;
    int64_t key = 0;
};
int cn_cov_spec_queue(cornetto_accel_t *h, cornetto_cov_t *c, int32_t lo, int32_t hi, float low_mq, int32_t edge_len, int32_t min_ctg_len, int boring,
                      unsigned long long *p_cnt, CnCovSpec *S);
int cn_cov_spec_finish(cornetto_accel_t *h, cornetto_cov_t *c, CnCovSpec *S, cornetto_regpk_t **recs, int64_t *n_recs, int64_t **ctg_first);
int cn_cov_select_packed_impl(cornetto_accel_t *h, cornetto_cov_t *c, int32_t lo, int32_t hi, float low_mq, int32_t edge_len, int32_t min_ctg_len, int boring,
                              cornetto_regpk_t **recs, int64_t *n_recs, int64_t **ctg_first);

// The fused telomere scan (cornetto_telo_scan with hits) for a motif without a border, queued without its three synchronisations: the dense
// lists, the pairing and the two result copies are sized by the counts of the last scan of the same assembly with the same motif and
// threshold (cornetto_asm::tf_est_*), the counts are checked afterwards.  Same protocol as the pair above.
struct CnTeloSpec {
    bool queued = false;
    cornetto_hit_t *hits = nullptr;        // result buffer, hit_cap records being copied
    size_t hit_cap = 0;
    size_t seg_cap[4] = {0, 0, 0, 0};
    int4 *p_wins = nullptr;                // pinned staging of the windows, win_cap of them
    size_t win_cap = 0;
    unsigned long long *p_cnt = nullptr;   // pinned, 16 x u64, the caller's: [0..3] list totals, [4] overflow | error, [8] windows
};
int cn_telo_spec_queue(cornetto_accel_t *h, cornetto_asm_t *a, const char *motif, double thr_adj, unsigned long long *p_cnt, CnTeloSpec *S);
int cn_telo_spec_finish(cornetto_accel_t *h, cornetto_asm_t *a, const char *motif, double thr_adj, CnTeloSpec *S, cornetto_hit_t **hits, int64_t *n_hits,
                        cornetto_win_t **wins, int64_t *n_wins);
int cn_telo_scan_impl(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, double thr_adj, cornetto_hit_t **hits, int64_t *n_hits, cornetto_win_t **wins,
                      int64_t *n_wins);

// The mark bitmap of a telomere scan alone (1 bit per base: the bases covered by a telofind run of either strand), left on the device in the
// window layout of the assembly (cornetto_asm::d_tw_boff, d_tw_tiles, tw_n_tiles): written by tf_scan beside its matches for a motif without
// a border, built from the runs otherwise.  Synchronises.  telostats.hip turns it into the merged regions at the contig ends.
int cn_telo_marks_impl(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, const unsigned long long **d_marks);

// The two lists cornetto_telo_breaks (telobreaks_ivl.hip) reads, left on the device: neither is copied to the host, only its count is.  Both
// take the plain synchronous route of their public entry points (no one-go form, no estimate of the last call) without the timing
// bracket, and both synchronise.  A list stays valid until the next sdust / telofind call on the handle.
//   cn_sdust_list_impl   cornetto_sdust_asm(): the stitched intervals, by contig, then by start (sdust.hip's workspace); nullptr when n is 0
//   cn_telo_hits_impl    cornetto_telofind(): the runs of both strands (telo.hip's workspace).  A motif with a border (AAAA, ACACA) or of
//                        more than 32 bytes keeps its present route — the greedy runs are collected on the host — and the finished list is
//                        uploaded again: such motifs are not what a telomere search runs with.
// A cornetto_sdust_asm_begin() nobody finished is finished and dropped first; that runs a timing bracket of its own, so a caller with a
// bracket calls cn_sdust_drop_pending() BEFORE it opens it (cn_sdust_list_impl() drops too: a no-op then).
void cn_sdust_drop_pending(cornetto_accel_t *h);

// cornetto_text_inflate() over raw device pointers, without its checks and its timing bracket (inflate.hip): the bedgraph feeds inflate into
// their own text workspaces with it.  Every block must lie inside both buffers.  Synchronises the handle's stream.
int cn_bgzf_inflate_raw(cornetto_accel_t *h, const uint8_t *d_comp, uint8_t *d_out, const cornetto_bgzf_block_t *blocks, int64_t n_blocks, int64_t *first_bad);
// cornetto_text_deflate() over raw device pointers (deflate.hip): the BGZF members of d_src[0 .. n), cut every 65280 bytes, packed back to back from
// d_out on (room for 65536 bytes a member), the chain's length to the device word *d_total.  Queued on the handle's stream: nothing is waited for,
// staging and sizes live in the handle's workspaces (calls follow each other on that stream).
int cn_bgzf_deflate_queue(cornetto_accel_t *h, const uint8_t *d_src, int64_t n, uint8_t *d_out, unsigned long long *d_total);
// qmean_sum (qmean.hip) queued on the handle's stream: d_sum[r] += the weights of the bytes d_text[d_start[r] .. + d_len[r]) for r < n, out of
// the table of printed FASTQ characters (bam == 0) or of raw BAM qualities.  The ranges ascend and do not overlap; the caller has zeroed d_sum
// on the same stream; d_text is readable to the next multiple of 16 behind n_text.  Nothing is waited for.
int cn_qmean_sum(cornetto_accel_t *h, const uint8_t *d_text, int64_t n_text, const uint32_t *d_start, const uint32_t *d_len, int64_t n, int bam, unsigned long long *d_sum);
int cn_sdust_list_impl(cornetto_accel_t *h, const cornetto_asm_t *a, int32_t T, int32_t W, const cornetto_ivl_t **d_ivls, int64_t *n_ivls);
int cn_telo_hits_impl(cornetto_accel_t *h, const cornetto_asm_t *a, const char *motif, const cornetto_hit_t **d_hits, int64_t *n_hits);
