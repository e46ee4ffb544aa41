/* qmean.c — `seq -q FLOAT` (not in the reference): the mean-quality rule of include/cornetto_accel.h for every host loop of `seq` — the kseq
 * loop of `seq FILE`, --accel=no for --fastq and --bam, and the sequential reader that takes over from the device — as ONE function of the
 * printed quality string, with the weight table of the shared header: 64-bit integers, no floating point. */
#include "cli.h"

static int64_t qm_max_err = -1;
static uint64_t qm_printed[2] = {0, 0};

void cli_qmean_set(int64_t max_err) { qm_max_err = max_err; }

int64_t cli_qmean_max_err(void) { return qm_max_err; }

int cli_qmean_pass(const char *qual, size_t n_qual, int64_t n_bases)
{
    static const uint32_t E[CORNETTO_QUAL_MAX + 1] = CORNETTO_QUAL_WEIGHTS;
    if (qm_max_err < 0 || n_qual == 0) return 1;
    uint64_t sum = 0;
    for (size_t i = 0; i < n_qual; ++i) {
        const int q = (int)(unsigned char)qual[i] - 33;
        sum += E[q < 0 ? 0 : q > CORNETTO_QUAL_MAX ? CORNETTO_QUAL_MAX : q];
    }
    return sum <= (uint64_t)qm_max_err * (uint64_t)n_bases;
}

void cli_qmean_count(int64_t n_bases) { cli_qmean_add(1, n_bases); }

void cli_qmean_add(int64_t reads, int64_t bases)
{
    qm_printed[0] += (uint64_t)reads;
    qm_printed[1] += (uint64_t)bases;
}

void cli_qmean_printed(uint64_t printed[2])
{
    printed[0] = qm_printed[0];
    printed[1] = qm_printed[1];
}
