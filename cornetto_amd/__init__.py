"""cornetto_amd — MI355X-native implementation of cornetto's panel-creation hot path.

The product is native: ``libcornetto_hip.so`` (hand-written HIP kernels for gfx950 behind the C ABI of
``include/cornetto_accel.h``) and the C host CLI ``cornetto`` (``cornetto_amd/cli``).  This module is a thin
ctypes binding of that C ABI, used by the tests, ``bench.py`` and the multi-process drivers: plumbing, not
a second implementation.  There is no Python or CPU fallback — if the shared library is missing, import
of :func:`lib` fails loudly.
"""
import ctypes as C
import os

import numpy as np

__all__ = ["lib", "Accel", "bgzf_scan", "bam_header", "BGZF_DT", "BAMREC_DT", "BAMFQREC_DT", "BAM_SCAN_TILE", "FQSEQ_TILE", "KQV_TILE", "Kset", "FQREC_DT", "Bgzf", "FastqBlockError", "BamFormatError", "AccelError", "HIT_DT", "WIN_DT", "IVL_DT", "TELROW_DT", "HAP_ROW_DT", "khash_str_order", "panel_boring", "REG_DT", "REGREC_DT", "build",
           "LIB_PATH", "CLI_PATH"]

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_LIB_PATH = os.path.join(HERE, "libcornetto_hip_dev.so")   # the same sources with -DCN_DEV: the development switches (CORNETTO_SDUST_CHUNK, ...) exist in this build only
LIB_PATH = os.environ.get("CORNETTO_LIB") or os.path.join(HERE, "libcornetto_hip.so")    # (CORNETTO_LIB: another build of the same library — A/B runs of kernel variants on one box)
CLI_PATH = os.path.join(HERE, "cornetto")

HIT_DT = np.dtype([("ctg", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("end", "<i4")])
WIN_DT = np.dtype([("ctg", "<i4"), ("start", "<i4"), ("end", "<i4"), ("car", "<i4")])
IVL_DT = np.dtype([("ctg", "<i4"), ("start", "<i4"), ("finish", "<i4")])
TELROW_DT = np.dtype([("ctg", "<i4"), ("start", "<i4"), ("end", "<i4"), ("matched", "<i4")])
HAP_ROW_DT = np.dtype([("query", "<i4"), ("ctg", "<i4"), ("start", "<i4"), ("finish", "<i4")])
FQREC_DT = np.dtype([("head", "<i8"), ("seq", "<i8"), ("qual", "<i8"), ("len", "<i4"), ("name_len", "<i4"),
                     ("comment_len", "<i4"), ("keep", "<i4")])
EMITREC_DT = np.dtype([("ctg", "<i4"), ("rc", "<i4"), ("head", "<i8"), ("head_len", "<i8")])
FAREC_DT = np.dtype([("head", "<i8"), ("len", "<i8"), ("name_len", "<i4"), ("pad", "<i4")])
BGZF_DT = np.dtype([("src", "<i8"), ("dst", "<i8"), ("n_src", "<i4"), ("n_dst", "<i4"), ("crc", "<u4"), ("pad", "<i4")])
REG_DT = np.dtype([("st", "<i4"), ("end", "<i4"), ("depth", "<i4"), ("mq_depth", "<i4")])
REGREC_DT = np.dtype([("ctg", "<i4"), ("st", "<i4"), ("end", "<i4"), ("depth", "<i4"), ("mq_depth", "<i4")])
REGPK_DT = np.dtype([("st", "<i4"), ("depth", "<u2"), ("mq_depth", "<u2")])


class BgErr(C.Structure):
    """cornetto_bgerr_t (include/cornetto_accel.h); `file` stands where the padding in front of `record` was"""
    _fields_ = [("kind", C.c_int32), ("file", C.c_int32), ("record", C.c_int64), ("a", C.c_int32), ("b", C.c_int32)]


class BgSrc(C.Structure):
    """cornetto_bgsrc_t (include/cornetto_accel.h)"""
    _fields_ = [("text", C.c_char_p), ("n", C.c_int64), ("comp", C.c_void_p), ("blocks", C.c_void_p), ("n_blocks", C.c_int64)]


BG_BLOCK = 11  # kind of a damaged BGZF block in cornetto_bgerr_t / cornetto_bgrunerr_t


class Bgzf:
    """one depth file of Accel.bedgraph_ingest_src() / bedgraph_runs_ingest_src() as a BGZF blob: its blocks are handed over `per_feed` at a
    time (an int, or a list with the number of blocks of every feed, zeros allowed; what the list leaves over goes into one more feed)"""

    def __init__(self, blob, per_feed=1):
        self.blob, self.per_feed = bytes(blob), per_feed

    def counts(self, n_blocks):
        if isinstance(self.per_feed, int):
            k = max(1, self.per_feed)
            return [min(k, n_blocks - i) for i in range(0, n_blocks, k)] or [0]
        c = [int(x) for x in self.per_feed]
        assert sum(c) <= n_blocks
        return c + ([n_blocks - sum(c)] if sum(c) < n_blocks else [])


class BgRunErr(C.Structure):
    """cornetto_bgrunerr_t (include/cornetto_accel.h)"""
    _fields_ = [("kind", C.c_int32), ("file", C.c_int32), ("record", C.c_int64), ("a", C.c_int32), ("b", C.c_int32)]


class BamErr(C.Structure):
    """cornetto_bamerr_t (include/cornetto_accel.h)"""
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("pad", C.c_int32), ("record", C.c_int64)]


class BamDepthOpt(C.Structure):
    """cornetto_bamdepth_opt_t (include/cornetto_accel.h)"""
    _fields_ = [("min_mapq", C.c_int32), ("skip_flags", C.c_uint32), ("window", C.c_int64), ("records", C.c_int32), ("pad", C.c_int32)]


class BamFqOpt(C.Structure):
    """cornetto_bamfq_opt_t (include/cornetto_accel.h)"""
    _fields_ = [("min_len", C.c_int32), ("duplex", C.c_int32), ("window", C.c_int64), ("n_ref", C.c_int32), ("records", C.c_int32)]


class FqSeqOpt(C.Structure):
    """cornetto_fqseq_opt_t (include/cornetto_accel.h)"""
    _fields_ = [("min_len", C.c_int32), ("records", C.c_int32), ("window", C.c_int64)]


KSET_CN_BINS = 6  # CORNETTO_KSET_CN_BINS: the copy-number classes of Kset.spectrum()
KSET_COUNT_CAP, KSET_HIST_BINS = 65535, 1024  # CORNETTO_KSET_COUNT_CAP, CORNETTO_KSET_HIST_BINS: the counted sets of Accel.kset(channels=1 or 2)
KQV_TILE = 4096  # CORNETTO_KQV_TILE: bases per workgroup of kq_insert / kq_query (tests plant seams at its multiples)
FQSEQ_TILE = 16384  # CORNETTO_FQSEQ_TILE: output bytes per workgroup of fqseq_text (checked against the library when it is loaded)
BAMFQREC_DT = np.dtype([("offset", "<i8"), ("l_seq", "<i4"), ("flag", "<i4"), ("name_len", "<i4"), ("kept", "<i4")])
BAMREC_DT = np.dtype([("offset", "<i8"), ("ref_id", "<i4"), ("pos", "<i4"), ("mapq", "<i4"), ("flag", "<i4"), ("counted", "<i4"), ("n_ops", "<i4"), ("span", "<i8"),
                      ("bases", "<i8")])
BAM_SCAN_TILE = 4096  # CORNETTO_BAM_SCAN_TILE: positions per workgroup of the depth scan (checked against the library when it is loaded)
BGRUN_TILE = 4096     # CORNETTO_BGRUN_TILE: positions per workgroup of the run expansion (checked against the library when it is loaded)


class StepOpt(C.Structure):
    """cornetto_step_opt_t (include/cornetto_accel.h)"""
    _fields_ = [("motif", C.c_char_p), ("thr_adj", C.c_double), ("window_size", C.c_int32), ("window_inc", C.c_int32), ("low_cov", C.c_float),
                ("high_cov", C.c_float), ("low_mq", C.c_float), ("edge_len", C.c_int32), ("min_ctg_len", C.c_int32), ("boring", C.c_int32)]


class HapOpt(C.Structure):
    """cornetto_hap_opt_t (include/cornetto_accel.h)"""
    _fields_ = [("merge_dist", C.c_int32), ("flank", C.c_int32)]


SUMS_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint64), C.c_void_p)


class BedgraphFormatError(ValueError):
    """a check of the reference's get_depths() failed (kind / record / numbers as in cornetto_bgerr_t), or one of the run-length reader
    (cornetto_bgrunerr_t: `file` is 0 or 1 there, None for the per-base reader)"""

    def __init__(self, kind, record, a, b, file=None):
        super().__init__("bedgraph check %d failed at record %d (%d, %d)%s" % (kind, record, a, b, "" if file is None else " of file %d" % file))
        self.kind, self.record, self.a, self.b, self.file = kind, record, a, b, file


class BamFormatError(ValueError):
    """a check of the BAM reader failed (kind / record / numbers as in cornetto_bamerr_t; kind 7: the file has no BAM header)"""

    def __init__(self, kind, record, a, b):
        super().__init__("BAM check %d failed at record %d (%d, %d)" % (kind, record, a, b))
        self.kind, self.record, self.a, self.b = kind, record, a, b


class FastqBlockError(ValueError):
    """a BGZF block of the FASTQ file handed to Accel.fastq_seq() is not what its footer says: block = its index in the file; text, stats,
    records and rest cover the records that lie wholly in front of it; refeed = the status of one more feed (refused)"""

    def __init__(self, block):
        super().__init__("BGZF block %d is not what its footer says" % block)
        self.block = block


class AccelError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("cornetto_accel status %d: %s" % (status, msg))
        self.status = status


def build(verbose=False):
    """compile libcornetto_hip.so and the CLI in-tree (hipcc --offload-arch=gfx950)"""
    import subprocess
    subprocess.check_call(["make", "-C", HERE] + ([] if verbose else ["-s"]))


_libs = {}


def lib(dev=False):
    """the loaded C ABI; raises if the HIP library has not been built.  dev=True: the development build of the same sources
    (libcornetto_hip_dev.so, -DCN_DEV), the only one that reads the development switches from the environment — a second, independent copy
    of the library in the process (own handles, own result pool)"""
    path = DEV_LIB_PATH if dev else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `make -C cornetto_amd` (or __graft_entry__.build()); "
                          "there is no fallback implementation" % path)
    L = C.CDLL(path)
    L.path = path
    vp, i32, i64, cp = C.c_void_p, C.c_int32, C.c_int64, C.c_char_p
    pp = C.POINTER(vp)
    sig = {
        "cornetto_accel_device_count": (C.c_int, []),
        "cornetto_accel_open": (C.c_int, [pp, C.c_int, vp]),
        "cornetto_accel_close": (None, [vp]),
        "cornetto_accel_last_error": (cp, [vp]),
        "cornetto_accel_strerror": (cp, [C.c_int]),
        "cornetto_free": (None, [vp]),
        "cornetto_accel_last_timing": (C.c_int, [vp, C.POINTER(cp), C.POINTER(C.c_float), C.c_int]),
        "cornetto_accel_set_share": (C.c_int, [vp, C.c_int]),
        "cornetto_accel_boost": (C.c_int, [vp, C.c_int]),
        "cornetto_accel_launch_count": (C.c_uint64, [vp]),
        "cornetto_accel_set_lazy": (C.c_int, [vp, C.c_int]),
        "cornetto_accel_wait": (C.c_int, [vp]),
        "cornetto_accel_set_timing": (C.c_int, [vp, C.c_int]),
        "cornetto_accel_warm": (C.c_int, [vp, C.c_int]),
        "cornetto_accel_sdust_stats": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "cornetto_cov_select_merged": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "cornetto_ivl_merge": (C.c_int, [vp, vp, C.c_int64, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "cornetto_panel_defaults": (None, [vp]),
        "cornetto_panel_defaults_recreate": (None, [vp]),
        "cornetto_panel_boring": (C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "cornetto_hap_defaults": (None, [vp]),
        "cornetto_hap_fun": (C.c_int, [vp, vp, i32, vp, vp, i32, vp, pp, C.POINTER(i64)]),
        "cornetto_telobreaks": (C.c_int, [vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "cornetto_telo_breaks": (C.c_int, [vp, vp, cp, i32, i32, pp, C.POINTER(i64)]),
        "cornetto_telobreaks_ivl": (C.c_int, [vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "cornetto_khash_str_order": (C.c_int32, [C.POINTER(C.c_char_p), C.c_int32, vp, vp]),
        "cornetto_fastq_split": (C.c_int, [vp, vp, i64, C.c_int, i32, pp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), pp]),
        "cornetto_fasta_split": (C.c_int, [vp, vp, i64, C.c_int, pp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), pp]),
        "cornetto_text_open": (C.c_int, [vp, i64, pp]),
        "cornetto_text_free": (None, [vp, vp]),
        "cornetto_text_put": (C.c_int, [vp, vp, vp, i64, i64, C.c_int]),
        "cornetto_text_wait": (C.c_int, [vp, vp, C.c_int]),
        "cornetto_fasta_split_text": (C.c_int, [vp, vp, i64, C.c_int, pp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), pp]),
        "cornetto_bgzf_scan": (C.c_int, [vp, i64, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]),
        "cornetto_text_inflate": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(i64)]),
        "cornetto_text_gather": (C.c_int, [vp, vp, vp, vp, i64, vp]),
        "cornetto_text_deflate": (C.c_int, [vp, vp, i64, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "cornetto_emit_open": (C.c_int, [vp, vp, vp, i64, vp, i64, pp, C.POINTER(i64)]),
        "cornetto_emit_get": (C.c_int, [vp, vp, vp, i64, i64, C.c_int]),
        "cornetto_emit_wait": (C.c_int, [vp, vp, C.c_int]),
        "cornetto_emit_free": (None, [vp, vp]),
        "cornetto_asm_upload": (C.c_int, [vp, vp, vp, i32, pp]),
        "cornetto_asm_wrap": (C.c_int, [vp, vp, vp, vp, i32, pp]),
        "cornetto_asm_free": (None, [vp, vp]),
        "cornetto_telofind": (C.c_int, [vp, vp, cp, pp, C.POINTER(i64)]),
        "cornetto_telowin_threshold": (C.c_double, [C.c_double, C.c_double]),
        "cornetto_telowin": (C.c_int, [vp, vp, i64, vp, i32, C.c_double, pp, C.POINTER(i64)]),
        "cornetto_telo_scan": (C.c_int, [vp, vp, cp, C.c_double, pp, C.POINTER(i64), pp, C.POINTER(i64)]),
        "cornetto_telo_ends": (C.c_int, [vp, vp, cp, C.c_double, i32, i32, pp, C.POINTER(i64)]),
        "cornetto_sdust_asm": (C.c_int, [vp, vp, i32, i32, pp, C.POINTER(i64)]),
        "cornetto_sdust_asm_begin": (C.c_int, [vp, vp, i32, i32]),
        "cornetto_sdust_asm_end": (C.c_int, [vp, vp, i32, i32, pp, C.POINTER(i64)]),
        "cornetto_sdust": (C.POINTER(C.c_uint64), [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
        "cornetto_sdust_buf_init": (vp, [vp]),
        "cornetto_sdust_buf_destroy": (None, [vp]),
        "cornetto_sdust_core": (C.POINTER(C.c_uint64), [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), vp]),
        "cornetto_cov_upload": (C.c_int, [vp, vp, vp, vp, i32, pp]),
        "cornetto_cov_wrap": (C.c_int, [vp, vp, vp, vp, vp, i32, pp]),
        "cornetto_cov_free": (None, [vp, vp]),
        "cornetto_cov_shard": (C.c_int, [vp, vp, vp, vp, i32, pp]),
        "cornetto_n_reg": (i32, [i32, i32, i32]),
        "cornetto_regs_assert": (i32, [i32, i32, i32]),
        "cornetto_cov_prepare": (C.c_int, [vp, vp, i32, i32, C.POINTER(C.c_uint64)]),
        "cornetto_cov_regs": (C.c_int, [vp, vp, i32, vp]),
        "cornetto_cov_threshold": (i32, [C.c_float, i32]),
        "cornetto_cov_select": (C.c_int, [vp, vp, i32, i32, C.c_float, i32, i32, C.c_int, pp, C.POINTER(i64)]),
        "cornetto_cov_select_packed": (C.c_int, [vp, vp, i32, i32, C.c_float, i32, i32, C.c_int, pp, C.POINTER(i64), pp]),
        "cornetto_panel_step": (C.c_int, [vp, vp, vp, C.POINTER(StepOpt), vp, vp, C.POINTER(C.c_uint64), C.POINTER(i32), pp, C.POINTER(i64), pp, pp, C.POINTER(i64),
                                          pp, C.POINTER(i64)]),
        "cornetto_cov_n": (i32, [vp]),
        "cornetto_cov_lens": (C.POINTER(i32), [vp]),
        "cornetto_pinned_alloc": (vp, [C.c_size_t]),
        "cornetto_pinned_free": (None, [vp]),
        "cornetto_bgin_open": (C.c_int, [vp, pp]),
        "cornetto_bgin_close": (None, [vp, vp]),
        "cornetto_bgin_feed": (C.c_int, [vp, vp, cp, i64, cp, i64, C.c_int]),
        "cornetto_bgin_prefetch": (C.c_int, [vp, vp, cp, i64, cp, i64]),
        "cornetto_bgin_pending": (None, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "cornetto_bgin_unmatched_mq": (i64, [vp]),
        "cornetto_bgin_error": (C.POINTER(BgErr), [vp]),
        "cornetto_bgin_done": (C.c_int, [vp]),
        "cornetto_bgin_finish": (C.c_int, [vp, vp, pp, C.POINTER(i32), C.POINTER(C.POINTER(cp)), C.POINTER(i64)]),
        "cornetto_bgrun_tile": (i32, []),
        "cornetto_bgrun_open": (C.c_int, [vp, pp]),
        "cornetto_bgrun_close": (None, [vp, vp]),
        "cornetto_bgrun_feed": (C.c_int, [vp, vp, C.c_int, cp, i64, C.c_int]),
        "cornetto_bgrun_error": (C.POINTER(BgRunErr), [vp]),
        "cornetto_bgrun_finish": (C.c_int, [vp, vp, pp, C.POINTER(i32), C.POINTER(C.POINTER(cp)), C.POINTER(i64)]),
        "cornetto_bgin_feed_src": (C.c_int, [vp, vp, C.POINTER(BgSrc), C.POINTER(BgSrc), C.c_int]),
        "cornetto_bgrun_feed_src": (C.c_int, [vp, vp, C.c_int, C.POINTER(BgSrc), C.c_int]),
        "cornetto_cov_download": (C.c_int, [vp, vp, i32, vp, vp]),
        "cornetto_bam_header": (C.c_int, [vp, i64, C.POINTER(i32), C.POINTER(C.POINTER(cp)), C.POINTER(C.POINTER(i32)), C.POINTER(i64)]),
        "cornetto_bamdepth_defaults": (None, [C.POINTER(BamDepthOpt)]),
        "cornetto_bam_scan_tile": (i32, []),
        "cornetto_bamdepth_open": (C.c_int, [vp, C.POINTER(BamDepthOpt), vp, i32, pp]),
        "cornetto_bamdepth_close": (None, [vp, vp]),
        "cornetto_bamdepth_feed": (C.c_int, [vp, vp, vp, vp, i64, i64]),
        "cornetto_bamdepth_error": (C.POINTER(BamErr), [vp]),
        "cornetto_bamdepth_finish": (C.c_int, [vp, vp, pp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "cornetto_bam_records": (C.c_int, [vp, vp, pp, C.POINTER(i64)]),
        "cornetto_bamfq_defaults": (None, [C.POINTER(BamFqOpt)]),
        "cornetto_bamfq_open": (C.c_int, [vp, C.POINTER(BamFqOpt), pp]),
        "cornetto_bamfq_close": (None, [vp, vp]),
        "cornetto_bamfq_feed": (C.c_int, [vp, vp, vp, vp, i64, i64, C.POINTER(i64), C.POINTER(i64)]),
        "cornetto_bamfq_get": (C.c_int, [vp, vp, vp, i64, i64, C.c_int]),
        "cornetto_bamfq_wait": (C.c_int, [vp, vp, C.c_int]),
        "cornetto_bamfq_get_bgzf": (C.c_int, [vp, vp, vp, i64, i64, i64, C.c_int]),
        "cornetto_bamfq_wait_bgzf": (C.c_int, [vp, vp, C.c_int, C.POINTER(i64)]),
        "cornetto_bamfq_finish": (C.c_int, [vp, vp]),
        "cornetto_bamfq_stats": (None, [vp, C.POINTER(i64)]),
        "cornetto_bamfq_error": (C.POINTER(BamErr), [vp]),
        "cornetto_bamfq_records": (C.c_int, [vp, vp, pp, C.POINTER(i64)]),
        "cornetto_bamfq_set_max_err": (C.c_int, [vp, vp, i64]),
        "cornetto_bamfq_qstats": (None, [vp, C.POINTER(i64)]),
        "cornetto_bamfq_qsums": (C.c_int, [vp, vp, pp, C.POINTER(i64)]),
        "cornetto_qual_weight": (C.c_uint32, [C.c_int]),
        "cornetto_fqseq_set_max_err": (C.c_int, [vp, vp, i64]),
        "cornetto_fqseq_qstats": (None, [vp, C.POINTER(i64)]),
        "cornetto_fqseq_qsums": (C.c_int, [vp, vp, pp, C.POINTER(i64)]),
        "cornetto_fqseq_tile": (i32, []),
        "cornetto_fqseq_defaults": (None, [C.POINTER(FqSeqOpt)]),
        "cornetto_fqseq_open": (C.c_int, [vp, C.POINTER(FqSeqOpt), pp]),
        "cornetto_fqseq_close": (None, [vp, vp]),
        "cornetto_fqseq_feed": (C.c_int, [vp, vp, C.POINTER(BgSrc), C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]),
        "cornetto_fqseq_rest": (i64, [vp]),
        "cornetto_fqseq_error": (i64, [vp]),
        "cornetto_fqseq_get": (C.c_int, [vp, vp, vp, i64, i64, C.c_int]),
        "cornetto_fqseq_wait": (C.c_int, [vp, vp, C.c_int]),
        "cornetto_fqseq_get_bgzf": (C.c_int, [vp, vp, vp, i64, i64, i64, C.c_int]),
        "cornetto_fqseq_wait_bgzf": (C.c_int, [vp, vp, C.c_int, C.POINTER(i64)]),
        "cornetto_fqseq_stats": (None, [vp, C.POINTER(i64)]),
        "cornetto_fqseq_records": (C.c_int, [vp, vp, pp, C.POINTER(i64)]),
        "cornetto_fqseq_text_time": (C.c_int, [vp, vp, C.POINTER(C.c_double), C.POINTER(i64)]),
        "cornetto_kset_open": (C.c_int, [vp, i32, i64, pp]),
        "cornetto_kset_add": (C.c_int, [vp, vp, vp]),
        "cornetto_kset_stats": (None, [vp, C.POINTER(i64)]),
        "cornetto_kset_query": (C.c_int, [vp, vp, vp, C.POINTER(i64), C.POINTER(i64), pp, C.POINTER(i64)]),
        "cornetto_kset_free": (None, [vp, vp]),
        "cornetto_kset_add_tag": (C.c_int, [vp, vp, vp, i32]),
        "cornetto_kset_phase": (C.c_int, [vp, vp, vp, C.POINTER(i64)]),
        "cornetto_kset_open_counted": (C.c_int, [vp, i32, i64, i32, pp]),
        "cornetto_kset_count": (C.c_int, [vp, vp, vp, i32]),
        "cornetto_kset_hist": (C.c_int, [vp, vp, i32, C.POINTER(i64)]),
        "cornetto_kset_seal": (C.c_int, [vp, vp, C.POINTER(i32), C.POINTER(i64)]),
        "cornetto_kset_copies": (C.c_int, [vp, vp, vp]),
        "cornetto_kset_copies_clear": (C.c_int, [vp, vp]),
        "cornetto_kset_spectrum": (C.c_int, [vp, vp, i32, i32, C.POINTER(i64), C.POINTER(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    assert L.cornetto_bgrun_tile() == BGRUN_TILE
    assert L.cornetto_bam_scan_tile() == BAM_SCAN_TILE
    assert L.cornetto_fqseq_tile() == FQSEQ_TILE
    L._declared = sorted(sig)
    _libs[path] = L
    return L


def bam_header(data):
    """cornetto_bam_header() over `data`, the first inflated bytes of a BAM -> (names, lens, header bytes), or None when the header goes on
    behind them; ValueError when they are no BAM header.  Host only."""
    L = lib()
    keep = np.frombuffer(bytes(data), dtype=np.uint8)
    n_ref, names, lens, hb = C.c_int32(), C.POINTER(C.c_char_p)(), C.POINTER(C.c_int32)(), C.c_int64()
    rc = L.cornetto_bam_header(keep.ctypes.data if keep.size else None, keep.size, C.byref(n_ref), C.byref(names), C.byref(lens), C.byref(hb))
    if rc == 1:
        return None
    if rc == -6:
        raise ValueError("not a BAM header")
    if rc != 0:
        raise AccelError(rc, L.cornetto_accel_strerror(rc).decode())
    nm = [names[i].decode() for i in range(n_ref.value)]
    ln = [lens[i] for i in range(n_ref.value)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    arr = C.cast(names, C.POINTER(C.c_void_p))
    for i in range(n_ref.value):
        libc.free(arr[i])
    libc.free(C.cast(names, C.c_void_p))
    libc.free(C.cast(lens, C.c_void_p))
    return nm, ln, hb.value


def bgzf_scan(data, file_off=0, dst=0):
    """cornetto_bgzf_scan() over `data`, the bytes at file_off of a BGZF file -> (blocks BGZF_DT: the members that lie wholly inside `data`, with
    dst counting on from `dst`; file offset to resume at; True if what begins there is not a BGZF member).  Host only."""
    L = lib()
    keep = np.frombuffer(bytes(data), dtype=np.uint8)
    blocks = np.zeros(keep.size // 26 + 1, dtype=BGZF_DT)
    d, nb, resume, broken = C.c_int64(dst), C.c_int64(), C.c_int64(), C.c_int32()
    rc = L.cornetto_bgzf_scan(keep.ctypes.data if keep.size else None, keep.size, file_off, C.byref(d), blocks.ctypes.data, blocks.size, C.byref(nb),
                              C.byref(resume), C.byref(broken))
    if rc != 0:
        raise AccelError(rc, L.cornetto_accel_strerror(rc).decode())
    return blocks[:nb.value].copy(), resume.value, bool(broken.value)


class _Owner:
    """keeps a library-owned result buffer alive for the numpy view over it; released with cornetto_free()"""

    def __init__(self, L, ptr):
        self.L, self.ptr = L, ptr

    def __del__(self):
        try:
            if self.ptr:
                self.L.cornetto_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def _take(L, ptr, n, dt):
    """zero-copy numpy view of a result array owned by library L (freed when the array is garbage collected)"""
    if not n:
        L.cornetto_free(ptr)
        return np.zeros(0, dtype=dt)
    addr = ptr.value if isinstance(ptr, C.c_void_p) else int(ptr)
    buf = (C.c_char * (n * dt.itemsize)).from_address(addr)
    buf._owner = _Owner(L, addr)          # the ctypes array is the numpy base; the owner dies with it
    return np.frombuffer(buf, dtype=dt)


class _Resident:
    def __init__(self, acc, ptr, free, lens):
        self.acc, self.ptr, self._free, self.lens = acc, ptr, free, list(lens)

    def close(self):
        if self.ptr is not None:
            self._free(self.acc.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Kset:
    """a set of canonical k-mers resident in HBM (cornetto_kset_*): Accel.kset(k, slots); with channels = 1 or 2 a counted set, which takes
    count() and hist() until seal() makes it the plain (1 channel) or the tagged (2) set that query() / phase() probe; a counted set of one
    channel also takes copies(), copies_clear() and spectrum() before its seal: completeness and the copy-number spectrum of an assembly"""

    def __init__(self, acc, ptr, k, slots, channels=0):
        self.acc, self.ptr, self.k, self.slots, self.channels = acc, ptr, k, slots, channels

    def count(self, asm, channel=0):
        """the k-mers of every record of the resident batch counted into `channel` (cornetto_kset_count); status -4 when the table overflowed"""
        self.acc._chk(self.acc.L.cornetto_kset_count(self.acc.h, self.ptr, asm.ptr, channel))

    def hist(self, channel=0):
        """-> int64[1024]: hist[c] = distinct k-mers of `channel` with min(count, 1023) == c; bin 0 stays 0 (cornetto_kset_hist)"""
        out = np.zeros(KSET_HIST_BINS, dtype=np.int64)
        self.acc._chk(self.acc.L.cornetto_kset_hist(self.acc.h, self.ptr, channel, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def copies(self, asm):
        """the k-mers of every contig of the resident assembly into the copy counts of a one-channel counted set, before its seal
        (cornetto_kset_copies); a k-mer the reads never held takes a slot with count 0; status -4 when the table overflowed"""
        self.acc._chk(self.acc.L.cornetto_kset_copies(self.acc.h, self.ptr, asm.ptr))

    def copies_clear(self):
        """every copy count back to 0; the keys stay (cornetto_kset_copies_clear)"""
        self.acc._chk(self.acc.L.cornetto_kset_copies_clear(self.acc.h, self.ptr))

    def spectrum(self, min_count, channel=0):
        """-> (int64[6, 1024], solid, found): spec[a, c] = keys with min(copies, 5) == a and min(count, 1023) == c; solid = keys with count >=
        min_count, found = those of them with a copy (cornetto_kset_spectrum)"""
        spec, tot = np.zeros((KSET_CN_BINS, KSET_HIST_BINS), dtype=np.int64), (C.c_int64 * 2)()
        self.acc._chk(self.acc.L.cornetto_kset_spectrum(self.acc.h, self.ptr, channel, int(min_count), spec.ctypes.data_as(C.POINTER(C.c_int64)), tot))
        return spec, int(tot[0]), int(tot[1])

    def seal(self, min_count):
        """min_count: an int, or one per channel -> the solid k-mers per channel; the set is plain or tagged from here on (cornetto_kset_seal)"""
        n = max(self.channels, 1)
        m = [int(min_count)] * n if np.isscalar(min_count) else [int(x) for x in min_count]
        if len(m) != n:
            raise ValueError("seal: %d thresholds for %d channels" % (len(m), n))
        mc, solid = (C.c_int32 * 2)(*m), (C.c_int64 * 2)()
        self.acc._chk(self.acc.L.cornetto_kset_seal(self.acc.h, self.ptr, mc, solid))
        return tuple(int(solid[i]) for i in range(n))

    def add(self, asm, tag=0):
        """the k-mers of every contig of the resident assembly into the set; AccelError with status -4 when the table overflowed.  tag 1 (pat) or
        2 (mat): into a tagged set (cornetto_kset_add_tag), the table of `cornetto trioeval`; a set is either plain or tagged"""
        if tag:
            self.acc._chk(self.acc.L.cornetto_kset_add_tag(self.acc.h, self.ptr, asm.ptr, tag))
        else:
            self.acc._chk(self.acc.L.cornetto_kset_add(self.acc.h, self.ptr, asm.ptr))

    @property
    def stats(self):
        """(positions inserted, distinct k-mers, slots)"""
        st = (C.c_int64 * 3)()
        self.acc.L.cornetto_kset_stats(self.ptr, st)
        return tuple(int(x) for x in st)

    def query(self, asm, runs=False):
        """-> (kmers, missing) int64 per contig of `asm`; with runs also the merged spans of the missing positions (IVL_DT)"""
        n = len(asm.lens)
        km, ms = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        p, nr = C.c_void_p(), C.c_int64()
        self.acc._chk(self.acc.L.cornetto_kset_query(self.acc.h, self.ptr, asm.ptr, km.ctypes.data_as(C.POINTER(C.c_int64)), ms.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     C.byref(p) if runs else None, C.byref(nr) if runs else None))
        if runs:
            return km[:n], ms[:n], _take(self.acc.L, p, nr.value, IVL_DT)
        return km[:n], ms[:n]

    def phase(self, asm):
        """-> (n, 7) int64 per contig of `asm` against a tagged set: kmers, pat, mat, pp, pm, mp, mm (cornetto_kset_phase)"""
        n = len(asm.lens)
        out = np.zeros((max(n, 1), 7), dtype=np.int64)
        self.acc._chk(self.acc.L.cornetto_kset_phase(self.acc.h, self.ptr, asm.ptr, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out[:n]

    def close(self):
        if self.ptr is not None:
            self.acc.L.cornetto_kset_free(self.acc.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accel:
    """one device + stream; mirrors the handle of include/cornetto_accel.h"""

    def __init__(self, device=0, stream=None, dev=False):
        self.L = lib(dev)
        self.lib_path = self.L.path                     # the library this handle runs: LIB_PATH, or DEV_LIB_PATH with dev=True
        h = C.c_void_p()
        rc = self.L.cornetto_accel_open(C.byref(h), device, stream)
        if rc != 0:
            raise AccelError(rc, self.L.cornetto_accel_strerror(rc).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.cornetto_accel_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise AccelError(rc, self.L.cornetto_accel_last_error(self.h).decode() or
                             self.L.cornetto_accel_strerror(rc).decode())

    def launch_count(self):
        """launches of resident sdust waves on this handle so far: cornetto_accel_launch_count()"""
        return int(self.L.cornetto_accel_launch_count(self.h))

    def set_lazy(self, on=True):
        """large result copies on a stream of their own; the arrays the calls return hold their content after wait(): cornetto_accel_set_lazy()"""
        self._chk(self.L.cornetto_accel_set_lazy(self.h, 1 if on else 0))

    def wait(self):
        self._chk(self.L.cornetto_accel_wait(self.h))

    def boost(self, on=True):
        """the rest of the device is free (on) / in use again (off): see cornetto_accel_boost(); callable from another thread"""
        self.L.cornetto_accel_boost(self.h, 1 if on else 0)

    def set_share(self, percent):
        """percent of every CU the resident sdust kernel may occupy (another handle computes beside this one)"""
        self._chk(self.L.cornetto_accel_set_share(self.h, int(percent)))

    def set_timing(self, level):
        self._chk(self.L.cornetto_accel_set_timing(self.h, level))

    def last_timing(self):
        """[(kernel name, ms)] of the most recent compute call (HIP events on the handle's stream)"""
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self.L.cornetto_accel_last_timing(self.h, names, ms, 64)
        return [(names[i].decode(), float(ms[i])) for i in range(min(n, 64))]

    # ---- sequences -------------------------------------------------------------------------------
    def asm_upload(self, seqs):
        """seqs: list of bytes / uint8 arrays -> resident assembly"""
        arrs = [np.frombuffer(bytes(s), dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else
                np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        n = len(arrs)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.int64)
        out = C.c_void_p()
        self._chk(self.L.cornetto_asm_upload(self.h, ptrs, lens.ctypes.data, n, C.byref(out)))
        return _Resident(self, out, self.L.cornetto_asm_free, lens)

    def kset(self, k=21, slots=1, channels=0):
        """an empty k-mer set with `slots` slots of 8 bytes: cornetto_kset_open(); channels = 1 or 2: a counted set with 4 more bytes per slot
        and channel (cornetto_kset_open_counted)"""
        out = C.c_void_p()
        if channels:
            self._chk(self.L.cornetto_kset_open_counted(self.h, k, slots, channels, C.byref(out)))
        else:
            self._chk(self.L.cornetto_kset_open(self.h, k, slots, C.byref(out)))
        return Kset(self, out, k, slots, channels)

    def asm_wrap(self, dev_ptr, offsets, lens):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        out = C.c_void_p()
        self._chk(self.L.cornetto_asm_wrap(self.h, dev_ptr, offsets.ctypes.data, lens.ctypes.data, len(lens), C.byref(out)))
        return _Resident(self, out, self.L.cornetto_asm_free, lens)

    def emit(self, asm, recs, heads, windows, slots=4):
        """the fixasm output text of `asm` (cornetto_emit_*): recs = [(ctg, rc, head, head_len)] (EMITREC_DT fields), heads = the header bytes
        -> (total bytes of the text, [bytes of every (at, n) of `windows`]); the windows go round the slots, each through a pinned buffer"""
        r = np.array([tuple(x) for x in recs], dtype=EMITREC_DT) if len(recs) else np.zeros(1, dtype=EMITREC_DT)
        hb = np.frombuffer(bytes(heads), dtype=np.uint8) if len(heads) else np.zeros(1, dtype=np.uint8)
        e, total = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_emit_open(self.h, asm.ptr, r.ctypes.data, len(recs), hb.ctypes.data, len(heads), C.byref(e), C.byref(total)))
        out, pins, pend = [], [None] * slots, [None] * slots
        try:
            for k, (at, n) in enumerate(windows):
                s = k % slots
                if pend[s] is not None:
                    self._chk(self.L.cornetto_emit_wait(self.h, e, s))
                    out[pend[s]] = C.string_at(pins[s], out[pend[s]])
                    self.L.cornetto_pinned_free(pins[s])
                pins[s] = self.L.cornetto_pinned_alloc(max(1, n))
                if not pins[s]:
                    raise MemoryError("cornetto_pinned_alloc(%d)" % n)
                self._chk(self.L.cornetto_emit_get(self.h, e, pins[s], at, n, s))
                pend[s] = len(out)
                out.append(n)
            for s in range(slots):
                if pend[s] is not None:
                    self._chk(self.L.cornetto_emit_wait(self.h, e, s))
                    out[pend[s]] = C.string_at(pins[s], out[pend[s]])
                    pend[s] = None
        finally:
            for s in range(slots):
                if pend[s] is not None:
                    self.L.cornetto_emit_wait(self.h, e, s)
            self.L.cornetto_emit_free(self.h, e)
            for p in pins:
                if p:
                    self.L.cornetto_pinned_free(p)
        return total.value, out

    def fastq_split(self, text, final=True, min_len=0, want_reads=False):
        """text: bytes-like FASTQ piece (or (address, size) of e.g. pinned memory) -> (records FQREC_DT, consumed bytes,
        plain flag, resident reads or None): see cornetto_fastq_split() in include/cornetto_accel.h"""
        if isinstance(text, tuple):
            addr, n = text
            keep = None
        else:
            keep = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
            addr, n = keep.ctypes.data, keep.size
        p, cnt, used, plain, reads = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_void_p()
        self._chk(self.L.cornetto_fastq_split(self.h, addr, n, 1 if final else 0, min_len, C.byref(p), C.byref(cnt), C.byref(used),
                                              C.byref(plain), C.byref(reads) if want_reads else None))
        recs = _take(self.L, p, cnt.value, FQREC_DT)
        res = _Resident(self, reads, self.L.cornetto_asm_free, recs["len"][recs["keep"] == 1]) if want_reads else None
        return recs, used.value, bool(plain.value), res

    def warm(self, what=7):
        """cornetto_accel_warm(): every entry point of the groups (1 sdust, 2 telo, 4 coverage) once on a built-in 4 kb input"""
        self._chk(self.L.cornetto_accel_warm(self.h, what))

    def fasta_split(self, text, final=True, want_seqs=False):
        """text: bytes-like FASTA piece beginning with '>' (or (address, size)) -> (records FAREC_DT, consumed bytes, plain
        flag, resident sequences or None): see cornetto_fasta_split() in include/cornetto_accel.h"""
        if isinstance(text, tuple):
            addr, n = text
            keep = None
        else:
            keep = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
            addr, n = keep.ctypes.data, keep.size
        p, cnt, used, plain, seqs = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_void_p()
        self._chk(self.L.cornetto_fasta_split(self.h, addr, n, 1 if final else 0, C.byref(p), C.byref(cnt), C.byref(used), C.byref(plain),
                                              C.byref(seqs) if want_seqs else None))
        recs = _take(self.L, p, cnt.value, FAREC_DT)
        res = _Resident(self, seqs, self.L.cornetto_asm_free, recs["len"]) if want_seqs else None
        return recs, used.value, bool(plain.value), res

    def fasta_split_slabs(self, text, slab_bytes, final=True, want_seqs=False):
        """the same through cornetto_text_open / _put / cornetto_fasta_split_text: `text` reaches the device in slabs of slab_bytes from a ring of
        four pinned slabs, out of order across the two copy queues"""
        keep = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        n = keep.size
        t = C.c_void_p()
        self._chk(self.L.cornetto_text_open(self.h, max(1, n), C.byref(t)))
        ring = [self.L.cornetto_pinned_alloc(slab_bytes) for _ in range(4)]
        try:
            offs = list(range(0, n, slab_bytes))
            order = offs[1::2] + offs[0::2]                  # (the device offsets are the caller's: any order)
            for k, at in enumerate(order):
                slot = k & 3
                if k >= 4:
                    self._chk(self.L.cornetto_text_wait(self.h, t, slot))
                m = min(slab_bytes, n - at)
                C.memmove(ring[slot], keep.ctypes.data + at, m)
                self._chk(self.L.cornetto_text_put(self.h, t, ring[slot], m, at, slot))
            p, cnt, used, plain, seqs = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_void_p()
            self._chk(self.L.cornetto_fasta_split_text(self.h, t, n, 1 if final else 0, C.byref(p), C.byref(cnt), C.byref(used), C.byref(plain),
                                                       C.byref(seqs) if want_seqs else None))
        finally:
            self.L.cornetto_text_free(self.h, t)
            for r in ring:
                self.L.cornetto_pinned_free(r)
        recs = _take(self.L, p, cnt.value, FAREC_DT)
        res = _Resident(self, seqs, self.L.cornetto_asm_free, recs["len"]) if want_seqs else None
        return recs, used.value, bool(plain.value), res

    def _text_from(self, data, cap=None):
        """`data` as a device text (cornetto_text_open + one cornetto_text_put from a pinned slab)"""
        keep = np.frombuffer(bytes(data), dtype=np.uint8)
        t = C.c_void_p()
        self._chk(self.L.cornetto_text_open(self.h, max(1, keep.size, cap or 0), C.byref(t)))
        if keep.size:
            pin = self.L.cornetto_pinned_alloc(keep.size)
            try:
                C.memmove(pin, keep.ctypes.data, keep.size)
                self._chk(self.L.cornetto_text_put(self.h, t, pin, keep.size, 0, 0))
                self._chk(self.L.cornetto_text_wait(self.h, t, 0))
            except Exception:
                self.L.cornetto_text_free(self.h, t)
                raise
            finally:
                self.L.cornetto_pinned_free(pin)
        return t

    def _text_bytes(self, t, n):
        """the first n bytes of a device text (cornetto_text_gather of one range)"""
        out = C.create_string_buffer(max(1, n))
        at, ln = np.array([0], dtype=np.int64), np.array([n], dtype=np.int32)
        self._chk(self.L.cornetto_text_gather(self.h, t, at.ctypes.data, ln.ctypes.data, 1, out))
        return out.raw[:n]

    def bgzf_inflate(self, data, blocks=None, fill=None):
        """the BGZF file `data` inflated on the device (cornetto_text_inflate) -> (bytes of the inflated text, first_bad: -1 or the index of the
        first block that is not what its footer says).  blocks: BGZF_DT, by default what bgzf_scan(data) gives (ValueError unless the chain
        ends with the data); fill: the inflated text and 256 bytes behind it are filled with this byte value beforehand and returned.  The status of the call is kept in
        self.last_status (0, or CORNETTO_E_FORMAT = -6 when first_bad >= 0), its kernel times in self.inflate_timing; every other status raises."""
        if blocks is None:
            blocks, resume, broken = bgzf_scan(data)
            if broken or resume != len(data):
                raise ValueError("not a BGZF chain: it ends at byte %d of %d" % (resume, len(data)))
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_DT)
        total = (int((blocks["dst"] + blocks["n_dst"]).max()) if blocks.size else 0) + (256 if fill is not None else 0)
        comp = self._text_from(data)
        out = None
        try:
            out = self._text_from(bytes([fill]) * total if fill is not None else b"", cap=total)
            bad = C.c_int64(-1)
            rc = self.L.cornetto_text_inflate(self.h, comp, out, blocks.ctypes.data, blocks.size, C.byref(bad))
            self.last_status, self.inflate_timing = rc, self.last_timing()      # (the copy below is a compute call of its own)
            if rc != 0 and not (rc == -6 and bad.value >= 0):
                self._chk(rc)
            return self._text_bytes(out, total), bad.value
        finally:
            self.L.cornetto_text_free(self.h, comp)
            if out is not None:
                self.L.cornetto_text_free(self.h, out)

    def bgzf_deflate(self, data, at=0, n=None, out_cap=None):
        """bytes [at, at + n) of `data` (by default: from `at` to its end) deflated into BGZF members on the device (cornetto_text_deflate:
        text_open, put, deflate, gather) -> the bytes of the chain, a member for every 65280 bytes, no end-of-file block.  out_cap: the
        capacity of the output text (by default what the call asks for: 65536 bytes a member).  The kernel times are kept in
        self.deflate_timing, the number of members in self.deflate_members."""
        n = len(data) - at if n is None else n
        n_mem = (n + 65279) // 65280
        text = self._text_from(data)
        out = None
        try:
            out = self._text_from(b"", cap=n_mem * 65536 if out_cap is None else out_cap)
            n_out, members = C.c_int64(-1), C.c_int64(-1)
            self._chk(self.L.cornetto_text_deflate(self.h, text, at, n, out, 0, C.byref(n_out), C.byref(members)))
            self.deflate_timing, self.deflate_members = self.last_timing(), members.value
            return self._text_bytes(out, n_out.value) if n_out.value else b""
        finally:
            self.L.cornetto_text_free(self.h, text)
            if out is not None:
                self.L.cornetto_text_free(self.h, out)

    def fasta_split_bgzf(self, data, final=True, want_seqs=False, want_names=False):
        """fasta_split_slabs() of the text the BGZF file `data` holds: inflated on the device (cornetto_text_inflate), framed there
        (cornetto_fasta_split_text) -> (records, consumed, plain, resident sequences or None); want_names: a fifth item, the records' names
        fetched with cornetto_text_gather.  A block that is not what its footer says raises AccelError (status -6)."""
        blocks, resume, broken = bgzf_scan(data)
        if broken or resume != len(data):
            raise ValueError("not a BGZF chain: it ends at byte %d of %d" % (resume, len(data)))
        total = int(blocks["n_dst"].sum())
        comp = self._text_from(data)
        out = None
        try:
            out = self._text_from(b"", cap=total)
            bad = C.c_int64(-1)
            self._chk(self.L.cornetto_text_inflate(self.h, comp, out, blocks.ctypes.data, blocks.size, C.byref(bad)))
            p, cnt, used, plain, seqs = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_void_p()
            self._chk(self.L.cornetto_fasta_split_text(self.h, out, total, 1 if final else 0, C.byref(p), C.byref(cnt), C.byref(used), C.byref(plain),
                                                       C.byref(seqs) if want_seqs else None))
            recs = _take(self.L, p, cnt.value, FAREC_DT)
            res = _Resident(self, seqs, self.L.cornetto_asm_free, recs["len"]) if want_seqs else None
            names = None
            if want_names:
                at = np.ascontiguousarray(recs["head"] + 1, dtype=np.int64)
                ln = np.ascontiguousarray(recs["name_len"], dtype=np.int32)
                buf = C.create_string_buffer(max(1, int(ln.sum())))
                self._chk(self.L.cornetto_text_gather(self.h, out, at.ctypes.data, ln.ctypes.data, len(recs), buf))
                ends = np.cumsum(ln)
                names = [buf.raw[int(e - k):int(e)] for e, k in zip(ends, ln)]
        finally:
            self.L.cornetto_text_free(self.h, comp)
            if out is not None:
                self.L.cornetto_text_free(self.h, out)
        return (recs, used.value, bool(plain.value), res) + ((names,) if want_names else ())

    # ---- telofind / telowin ----------------------------------------------------------------------
    def telofind(self, asm, motif=b"TTAGGG"):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telofind(self.h, asm.ptr, motif, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, HIT_DT)

    def telowin_threshold(self, thr, identity):
        return self.L.cornetto_telowin_threshold(thr, identity)

    def telowin(self, hits, ctg_len, thr_adj):
        hits = np.ascontiguousarray(hits, dtype=HIT_DT)
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telowin(self.h, hits.ctypes.data, hits.size, ctg_len.ctypes.data, ctg_len.size,
                                          thr_adj, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, WIN_DT)

    def telo_scan(self, asm, motif, thr_adj, want_hits=True):
        ph, nh, pw, nw = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telo_scan(self.h, asm.ptr, motif, thr_adj,
                                            C.byref(ph) if want_hits else None, C.byref(nh) if want_hits else None,
                                            C.byref(pw), C.byref(nw)))
        hits = _take(self.L, ph, nh.value, HIT_DT) if want_hits else None
        return hits, _take(self.L, pw, nw.value, WIN_DT)

    def telo_ends(self, asm, motif, thr_adj, merge_dist=100, ends=50000):
        """cornetto_telo_ends(): the telomere regions at the contig ends (the rows of scripts/telostats.sh's BED) -> IVL_DT rows
        (ctg, start, finish), a region once per end interval of its contig that it overlaps"""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telo_ends(self.h, asm.ptr, motif, thr_adj, merge_dist, ends, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    # ---- sdust -----------------------------------------------------------------------------------
    def sdust(self, asm, T=20, W=64):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_sdust_asm(self.h, asm.ptr, T, W, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def sdust_begin(self, asm, T=20, W=64):
        """cornetto_sdust_asm_begin(): queue the call without waiting where the last call's counts allow it (else nothing); sdust_end() delivers"""
        self._chk(self.L.cornetto_sdust_asm_begin(self.h, asm.ptr, T, W))

    def sdust_end(self, asm, T=20, W=64):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_sdust_asm_end(self.h, asm.ptr, T, W, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def sdust_stats(self, asm, T=20, W=64, intervals=False):
        """one extra sdust pass with the counting build of the kernel -> its counters as a dict (see
        cornetto_accel_sdust_stats() in include/cornetto_accel.h); None for parameters the production kernel does not take.
        intervals=True: -> (that, the intervals of the counting pass)"""
        self.L.cornetto_accel_sdust_stats(self.h, 1, None, 0)
        try:
            ivls = self.sdust(asm, T, W)
        finally:
            out = np.zeros(256, dtype=np.uint64)
            n = self.L.cornetto_accel_sdust_stats(self.h, 0, out.ctypes.data, 256)
        s = [int(x) for x in out[:n]]
        waves = s[254]
        if n > 207 and s[206]:
            # the sift / resolve kernel (csrc/sdust_sift.hpp): positions after each filter, steps of the stepping stages
            st = {"kernel": "sd_sift", "chunks": s[255], "tiles_of_64_bases": s[206], "positions_ct_above_T10": s[203], "after_L1": s[204], "after_L2": s[205],
                    "resolve_steps": s[200], "resolve_window_reads": s[201], "dp_tiles": s[208], "passes_with_candidates": s[202], "base_by_base_steps_of_chunks_with_other_bytes": s[207],
                    "window_reads_behind_a_gap_of": {"2": s[209], "3-4": s[210], "5-8": s[211]} if n > 211 else None,
                    # chunks handed out per counter request; chunks that took the seam tile over from the chunk before instead of redoing it
                    "chunks_per_group": s[213] if n > 213 else None, "seams_carried": s[212] if n > 213 else None}
            return (st, ivls) if intervals else st
        if not waves or not s[2]:
            return (None, ivls) if intervals else None
        hist = []
        for b in range(32):
            w = s[16 + 4 * b]
            if w:
                hist.append({"ms": [b * 0.5, b * 0.5 + 0.5], "waves": w, "jobs": s[18 + 4 * b], "find_perfect": s[19 + 4 * b], "find_perfect_with_candidates": s[17 + 4 * b]})
        st = {"waves": waves, "chunks": s[255], "chunks_sampled_low_complexity": s[7], "wave_steps": s[2], "find_perfect_calls": s[3],
                "find_perfect_with_candidates": s[10], "plain_groups": s[4], "wave_ms_avg": round(s[5] / waves / 1e5, 3), "wave_ms_max": round(s[6] / 1e5, 3),
                "queue_fetch_rounds_per_wave": round(s[11] / waves, 1), "wave_time_histogram": hist}
        return (st, ivls) if intervals else st

    # ---- panel interval stage ---------------------------------------------------------------------
    def cov_select_merged(self, cov, lo, hi, low_mq, edge_len, min_ctg_len, boring, merge_dist=1000, min_len=30000):
        """cov_select + bedtools merge -d merge_dist + length filter, all on the device -> IVL_DT rows"""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_cov_select_merged(self.h, cov.ptr, lo, hi, low_mq, edge_len, min_ctg_len, 1 if boring else 0, merge_dist, min_len,
                                                    C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def ivl_merge(self, ivls, dist):
        ivls = np.ascontiguousarray(ivls, dtype=IVL_DT)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_ivl_merge(self.h, ivls.ctypes.data, len(ivls), dist, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def hap_fun(self, lens, rows_per_hap, merge_dist=None, flank=None):
        """cornetto_hap_fun(): the merged haplotype funbits of scripts/create-hapnetto.sh:40-67.  lens: int32 per contig of the assembly;
        rows_per_hap: one HAP_ROW_DT array per haplotype (query id, contig index, start, finish), rows in any order -> IVL_DT rows"""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        parts = [np.ascontiguousarray(r, dtype=HAP_ROW_DT).reshape(-1) for r in rows_per_hap]
        rows = np.concatenate(parts) if parts else np.zeros(0, HAP_ROW_DT)
        n_rows = np.array([len(r) for r in parts], dtype=np.int64)
        opt = HapOpt()
        self.L.cornetto_hap_defaults(C.byref(opt))
        if merge_dist is not None:
            opt.merge_dist = merge_dist
        if flank is not None:
            opt.flank = flank
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_hap_fun(self.h, lens.ctypes.data, len(lens), rows.ctypes.data, n_rows.ctypes.data, len(parts), C.byref(opt),
                                          C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    # ---- telobreaks ------------------------------------------------------------------------------
    def telobreaks(self, ctg_len, sd, tel):
        """ctg_len: int32 per contig; sd: IVL_DT rows (ctg, start, finish); tel: TELROW_DT rows -> IVL_DT rows
        {ctg, first - 1 clamped at 0, last} of the low-complexity runs holding a telomere row with its flanks"""
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        sd = np.ascontiguousarray(sd, dtype=IVL_DT)
        tel = np.ascontiguousarray(tel, dtype=TELROW_DT)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telobreaks(self.h, ctg_len.ctypes.data, len(ctg_len), sd.ctypes.data, len(sd), tel.ctypes.data, len(tel),
                                             C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def telobreaks_ivl(self, ctg_len, sd, tel):
        """cornetto_telobreaks_ivl(): the same records by the interval rule, for an sd list sorted by (ctg, start) whose starts lie beyond
        the previous finish (what sdust prints); AccelError -3 for a list that is not"""
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        sd = np.ascontiguousarray(sd, dtype=IVL_DT)
        tel = np.ascontiguousarray(tel, dtype=TELROW_DT)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telobreaks_ivl(self.h, ctg_len.ctypes.data, len(ctg_len), sd.ctypes.data, len(sd), tel.ctypes.data, len(tel),
                                                 C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    def telo_breaks(self, asm, motif=b"TTAGGG", T=20, W=64):
        """cornetto_telo_breaks(): sdust(T, W), telofind(motif) and the interval rule on a resident assembly -> IVL_DT rows, the records of
        telobreaks() on the two lists; neither list leaves the device"""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_telo_breaks(self.h, asm.ptr, motif, T, W, C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, IVL_DT)

    # ---- coverage --------------------------------------------------------------------------------
    def cov_upload(self, depths, mqs):
        d = [np.ascontiguousarray(x, dtype=np.uint16) for x in depths]
        q = [np.ascontiguousarray(x, dtype=np.uint16) for x in mqs]
        n = len(d)
        pd = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in d])
        pq = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in q])
        lens = np.array([a.size for a in d], dtype=np.int32)
        out = C.c_void_p()
        self._chk(self.L.cornetto_cov_upload(self.h, pd, pq, lens.ctypes.data, n, C.byref(out)))
        return _Resident(self, out, self.L.cornetto_cov_free, lens)

    def cov_wrap(self, d_depth, d_mq, offsets, lens):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        out = C.c_void_p()
        self._chk(self.L.cornetto_cov_wrap(self.h, d_depth, d_mq, offsets.ctypes.data, lens.ctypes.data, len(lens), C.byref(out)))
        return _Resident(self, out, self.L.cornetto_cov_free, lens)

    def cov_shard(self, src_acc, cov, ctgs):
        """contigs `ctgs` of `cov` (resident on src_acc's device) as a new coverage object on this handle's device"""
        ctgs = np.ascontiguousarray(ctgs, dtype=np.int32)
        out = C.c_void_p()
        self._chk(self.L.cornetto_cov_shard(src_acc.h, cov.ptr, self.h, ctgs.ctypes.data, len(ctgs), C.byref(out)))
        return _Resident(self, out, self.L.cornetto_cov_free, [cov.lens[i] for i in ctgs])

    def cov_prepare(self, cov, w=2500, inc=50):
        sums = (C.c_uint64 * 3)()
        self._chk(self.L.cornetto_cov_prepare(self.h, cov.ptr, w, inc, sums))
        cov.w, cov.inc = w, inc
        return int(sums[0]), int(sums[1]), int(sums[2])

    def cov_download(self, cov, ctg):
        """-> (depth, mq_depth) of contig `ctg`, position by position: cornetto_cov_download()"""
        d = np.zeros(int(cov.lens[ctg]), dtype=np.uint16)
        q = np.zeros(int(cov.lens[ctg]), dtype=np.uint16)
        self._chk(self.L.cornetto_cov_download(self.h, cov.ptr, ctg, d.ctypes.data, q.ctypes.data))
        return d, q

    def cov_regs(self, cov, ctg):
        n = self.L.cornetto_n_reg(int(cov.lens[ctg]), cov.w, cov.inc)
        out = np.zeros(n, dtype=REG_DT)
        self._chk(self.L.cornetto_cov_regs(self.h, cov.ptr, ctg, out.ctypes.data))
        return out

    def cov_threshold(self, factor, mean):
        return self.L.cornetto_cov_threshold(factor, mean)

    def cov_select(self, cov, lo, hi, low_mq, edge_len, min_ctg_len, boring):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cornetto_cov_select(self.h, cov.ptr, lo, hi, low_mq, edge_len, min_ctg_len, int(boring),
                                             C.byref(p), C.byref(n)))
        return _take(self.L, p, n.value, REGREC_DT)

    def cov_select_packed(self, cov, lo, hi, low_mq, edge_len, min_ctg_len, boring):
        """-> (REGPK_DT records {st, depth, mq_depth}, int64 ctg_first[n + 1]): the windows of contig i are
        recs[ctg_first[i]:ctg_first[i + 1]], end = min(st + w, len)"""
        p, n, cf = C.c_void_p(), C.c_int64(), C.c_void_p()
        self._chk(self.L.cornetto_cov_select_packed(self.h, cov.ptr, lo, hi, low_mq, edge_len, min_ctg_len, int(boring),
                                                    C.byref(p), C.byref(n), C.byref(cf)))
        return _take(self.L, p, n.value, REGPK_DT), _take(self.L, cf, len(cov.lens) + 1, np.dtype("<i8"))

    def panel_step(self, asm, cov, motif, thr_adj, w=2500, inc=50, low_cov=0.4, high_cov=2.5, low_mq=0.4, edge_len=100000, min_ctg_len=1000000, boring=False,
                   exchange=None):
        """cornetto_panel_step(): cov_prepare -> thresholds -> cov_select_packed -> telo_scan in one call with two synchronisations.
        exchange(sums) -> sums (three ints): the all-reduce over the ranks, or None.
        -> (sums, (lo, hi), packed records, ctg_first, hits, windows)"""
        opt = StepOpt(motif, thr_adj, w, inc, low_cov, high_cov, low_mq, edge_len, min_ctg_len, int(bool(boring)))
        box = {}

        def _x(ptr, _ctx):
            try:
                r = exchange((int(ptr[0]), int(ptr[1]), int(ptr[2])))
                ptr[0], ptr[1], ptr[2] = int(r[0]), int(r[1]), int(r[2])
                return 0
            except BaseException as e:      # (an exception must not travel through the C frames)
                box["err"] = e
                return 1
        cb = SUMS_FN(_x) if exchange is not None else None
        cb_p = C.cast(cb, C.c_void_p) if cb is not None else None
        sums = (C.c_uint64 * 3)()
        thr = (C.c_int32 * 2)()
        p, n, cf, ph, nh, pw, nw = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        rc = self.L.cornetto_panel_step(self.h, asm.ptr, cov.ptr, C.byref(opt), cb_p, None, sums, thr, C.byref(p), C.byref(n), C.byref(cf), C.byref(ph), C.byref(nh),
                                        C.byref(pw), C.byref(nw))
        if "err" in box:
            raise box["err"]
        self._chk(rc)
        cov.w, cov.inc = w, inc
        return ((int(sums[0]), int(sums[1]), int(sums[2])), (int(thr[0]), int(thr[1])), _take(self.L, p, n.value, REGPK_DT), _take(self.L, cf, len(cov.lens) + 1, np.dtype("<i8")),
                _take(self.L, ph, nh.value, HIT_DT), _take(self.L, pw, nw.value, WIN_DT))

    @staticmethod
    def unpack_regs(recs, ctg_first, lens, w):
        """packed selection -> REGREC_DT rows (ctg, st, end, depth, mq_depth)"""
        out = np.zeros(len(recs), dtype=REGREC_DT)
        counts = np.diff(np.asarray(ctg_first, dtype=np.int64))
        ctg = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
        out["ctg"] = ctg
        out["st"] = recs["st"]
        out["end"] = np.minimum(recs["st"].astype(np.int64) + w, np.asarray(lens, dtype=np.int64)[ctg]).astype(np.int32)
        out["depth"] = recs["depth"]
        out["mq_depth"] = recs["mq_depth"]
        return out

    # ---- bedgraph ingest ---------------------------------------------------------------------------
    def _ingested(self, cov, nc, names, ncl):
        """what cornetto_bgin_finish() / cornetto_bgrun_finish() hand over -> (resident coverage, [contig names], clamped count)"""
        L = self.L
        nm = [names[i] for i in range(nc.value)]
        lens = [L.cornetto_cov_lens(cov)[i] for i in range(nc.value)]
        # the name strings are malloc'd by the library: release them with libc free
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        arr = C.cast(names, C.POINTER(C.c_void_p))
        for i in range(nc.value):
            libc.free(arr[i])
        libc.free(C.cast(names, C.c_void_p))
        return _Resident(self, cov, L.cornetto_cov_free, lens), nm, ncl.value

    # ---- BAM ---------------------------------------------------------------------------------------
    def _bam_run(self, blob, window, min_mapq, records, feeds=1):
        """the BAM file `blob` through cornetto_bamdepth_*: the header from the leading blocks (zlib + cornetto_bam_header), the compressed
        bytes as one device text, its blocks in `feeds` feeds -> (names, coverage or None, record table or None, n_records, n_counted,
        n_clamped).  Raises BamFormatError; a record larger than the window raises AccelError (status -4).  The kernel times of all
        feeds and of the finish are kept in self.bam_timing."""
        import zlib
        L = self.L
        blocks, resume, broken = bgzf_scan(blob)
        if broken or resume != len(blob):
            raise BamFormatError(7 if not len(blocks) else 6, 0, 0, 0)
        head, hdr = b"", None
        for b in blocks:
            try:
                head += zlib.decompress(bytes(blob[int(b["src"]):int(b["src"]) + int(b["n_src"])]), -15)
            except zlib.error:
                raise BamFormatError(6, 0, 0, 0)
            try:
                hdr = bam_header(head)
            except ValueError:
                raise BamFormatError(7, -1, 0, 0)
            if hdr is not None:
                break
        if hdr is None:
            raise BamFormatError(2, -1, 0, -1)
        names, lens, skip = hdr
        opt = BamDepthOpt()
        L.cornetto_bamdepth_defaults(C.byref(opt))
        opt.min_mapq, opt.records = min_mapq, records
        if window is not None:
            opt.window = window
        lens_a = np.array(lens, dtype=np.int32)
        comp = self._text_from(blob)
        bd = C.c_void_p()
        self.bam_timing = []
        try:
            self._chk(L.cornetto_bamdepth_open(self.h, C.byref(opt), lens_a.ctypes.data, len(lens), C.byref(bd)))

            def check(rc):
                self.bam_timing += self.last_timing()
                if rc == -6:
                    e = L.cornetto_bamdepth_error(bd).contents
                    if e.kind:
                        raise BamFormatError(e.kind, e.record, e.a, e.b)
                self._chk(rc)
            cuts = [len(blocks) * i // feeds for i in range(feeds + 1)]
            for i in range(feeds):
                part = np.ascontiguousarray(blocks[cuts[i]:cuts[i + 1]])
                check(L.cornetto_bamdepth_feed(self.h, bd, comp, part.ctypes.data, part.size, skip if i == 0 else 0))
            cov, nr, nc, ncl = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
            check(L.cornetto_bamdepth_finish(self.h, bd, C.byref(cov), C.byref(nr), C.byref(nc), C.byref(ncl)))
            res = _Resident(self, cov, L.cornetto_cov_free, lens) if cov.value else None
            recs = None
            if records:
                p, n = C.c_void_p(), C.c_int64()
                self._chk(L.cornetto_bam_records(self.h, bd, C.byref(p), C.byref(n)))
                recs = _take(L, p, n.value, BAMREC_DT)
            return names, res, recs, nr.value, nc.value, ncl.value
        finally:
            if bd.value:
                L.cornetto_bamdepth_close(self.h, bd)
            L.cornetto_text_free(self.h, comp)

    def bam_depth(self, blob, window=None, min_mapq=20, feeds=1):
        """both coverage tracks of the BAM file `blob` (bytes) -> (resident coverage, [contig names], n_records, n_counted, n_clamped): what
        `samtools depth -aa` and `samtools depth -Q min_mapq -aa` count (include/cornetto_accel.h states the rules).  window: bytes of
        inflated BAM on the device at once (never changes a result); feeds: the blocks are handed over in that many calls."""
        names, cov, _, nr, nc, ncl = self._bam_run(blob, window, min_mapq, 0, feeds)
        return cov, names, nr, nc, ncl

    def bam_records(self, blob, window=None):
        """the records of the BAM file `blob` as the depth kernel reads them (BAMREC_DT); no depth array is allocated"""
        return self._bam_run(blob, window, 20, 2)[2]

    def _bam_head(self, blob):
        """the BGZF blocks of the BAM file `blob` and its header (zlib + cornetto_bam_header) -> (blocks, names, lens, header bytes)"""
        import zlib
        blocks, resume, broken = bgzf_scan(blob)
        if broken or resume != len(blob):
            raise BamFormatError(7 if not len(blocks) else 6, 0, 0, 0)
        head, hdr = b"", None
        for b in blocks:
            try:
                head += zlib.decompress(bytes(blob[int(b["src"]):int(b["src"]) + int(b["n_src"])]), -15)
            except zlib.error:
                raise BamFormatError(6, 0, 0, 0)
            try:
                hdr = bam_header(head)
            except ValueError:
                raise BamFormatError(7, -1, 0, 0)
            if hdr is not None:
                break
        if hdr is None:
            raise BamFormatError(2, -1, 0, -1)
        return (blocks,) + tuple(hdr)

    def bam_fastq(self, blob, min_len=0, duplex=False, window=None, slab=None, feeds=1, max_err=None):
        """the BAM file `blob` (bytes) through the feed / get loop of cornetto_bamfq_*: the FASTQ text `seq --bam` prints -> (text, stats,
        records): stats = [reads, bases of `total reads`, reads, bases of `reads >= min_len`], records = the record table (BAMFQREC_DT).
        window: bytes of inflated BAM on the device at once; slab: bytes per get (the whole text of a window by default), the gets take
        turns on the four copy slots; feeds: the blocks are handed over in that many parts.  Neither changes a result.  Raises
        BamFormatError, which carries text, stats and records of the records in front of the failing one; a record larger than the window
        raises AccelError (status -4).  The kernel times of the feeds are kept in self.bam_timing.  max_err: P of `seq -q` (an integer
        0 .. 10^9, None: off; cornetto_bamfq_set_max_err): `kept` of the records is then 1 for the printed ones, self.bam_qstats = [reads,
        bases printed] and self.bam_qsums = the records' sums of quality weights (uint64; None without max_err)."""
        L = self.L
        blocks, _names, lens, skip = self._bam_head(blob)
        comp = self._text_from(blob)
        fq = None
        pins, cap = [None] * 4, [0] * 4
        out = []
        self.bam_timing = []

        def result():
            st = (C.c_int64 * 5)()
            L.cornetto_bamfq_stats(fq, st)
            p, n = C.c_void_p(), C.c_int64()
            self._chk(L.cornetto_bamfq_records(self.h, fq, C.byref(p), C.byref(n)))
            qs = (C.c_int64 * 2)()
            L.cornetto_bamfq_qstats(fq, qs)
            self.bam_qstats, self.bam_qsums = list(qs), None
            if max_err is not None:
                ps, ns = C.c_void_p(), C.c_int64()
                self._chk(L.cornetto_bamfq_qsums(self.h, fq, C.byref(ps), C.byref(ns)))
                self.bam_qsums = _take(L, ps, ns.value, np.dtype(np.uint64))
            return b"".join(out), list(st)[:4], _take(L, p, n.value, BAMFQREC_DT)

        def fail():
            e = L.cornetto_bamfq_error(fq).contents
            err = BamFormatError(e.kind, e.record, e.a, e.b)
            err.text, err.stats, err.records = result()
            return err

        def pull(n_text):
            pend, at, k = [0] * 4, 0, 0
            while at < n_text or any(pend):
                s = k & 3
                k += 1
                if pend[s]:
                    self._chk(L.cornetto_bamfq_wait(self.h, fq, s))
                    out.append(C.string_at(pins[s], pend[s]))
                    pend[s] = 0
                if at < n_text:
                    n = min(slab or n_text, n_text - at)
                    if cap[s] < n:
                        if pins[s]:
                            L.cornetto_pinned_free(pins[s])
                        pins[s] = L.cornetto_pinned_alloc(n)
                        cap[s] = n
                        if not pins[s]:
                            raise MemoryError("cornetto_pinned_alloc(%d)" % n)
                    self._chk(L.cornetto_bamfq_get(self.h, fq, pins[s], at, n, s))
                    pend[s] = n
                    at += n
        try:
            opt = BamFqOpt()
            L.cornetto_bamfq_defaults(C.byref(opt))
            opt.min_len, opt.duplex, opt.n_ref, opt.records = min_len, int(bool(duplex)), len(lens), 1
            if window is not None:
                opt.window = window
            fq = C.c_void_p()
            self._chk(L.cornetto_bamfq_open(self.h, C.byref(opt), C.byref(fq)))
            if max_err is not None:
                self._chk(L.cornetto_bamfq_set_max_err(self.h, fq, max_err))
            cuts = [len(blocks) * i // feeds for i in range(feeds + 1)]
            for i in range(feeds):
                part = np.ascontiguousarray(blocks[cuts[i]:cuts[i + 1]])
                at, first = 0, True
                while at < part.size or (first and i == 0):
                    taken, n_text = C.c_int64(), C.c_int64()
                    rc = L.cornetto_bamfq_feed(self.h, fq, comp, part[at:].ctypes.data if at < part.size else None, part.size - at, skip if i == 0 and first else 0,
                                               C.byref(taken), C.byref(n_text))
                    self.bam_timing += self.last_timing()
                    first = False
                    if rc not in (0, -6):
                        self._chk(rc)
                    pull(n_text.value)
                    if rc == -6:
                        raise fail()
                    at += taken.value
                    if part.size == 0:
                        break
            rc = L.cornetto_bamfq_finish(self.h, fq)
            self.bam_timing += self.last_timing()          # (bamfq_text in all)
            if rc == -6 and L.cornetto_bamfq_error(fq).contents.kind:
                raise fail()
            self._chk(rc)
            return result()
        finally:
            for p in pins:
                if p:
                    L.cornetto_pinned_free(p)
            if fq is not None and fq.value:
                L.cornetto_bamfq_close(self.h, fq)
            L.cornetto_text_free(self.h, comp)

    def fastq_seq(self, data, min_len, window=None, slab=None, feeds=1, bgzf_in=False, bgzf_out=False, max_err=None):
        """FASTQ text through the feed / get loop of cornetto_fqseq_*: what `seq -m min_len` prints -> (text, stats, recs, rest_offset, plain).
        data: the text (bytes), or with bgzf_in the file as a BGZF blob (inflated on the device), or a list of parts of the stream, each
        bytes or a Bgzf (the kind may change between feeds); the bytes / blocks of every part are handed over in `feeds` parts.  text: the
        printed text — with bgzf_out the list of what every get returned (a chain of BGZF members each); stats = [reads, bases of `total
        reads`, reads, bases of `reads >= min_len`]; recs: the record table (FQREC_DT, offsets into the stream); rest_offset: the offset
        in the plain / inflated stream of the first byte the device did not consume; plain: False when the sequential reader has to go
        on from there.  window: bytes of text on the device at once; slab: bytes per get (the whole text of a window by default), the gets
        take turns on the four copy slots.  Neither changes a result.  Raises FastqBlockError for a damaged block; a record larger than the
        window raises AccelError (status -4, .taken = 0).  Kernel times of the feeds: self.fq_timing; of fqseq_text: self.fq_text_time =
        (ms, bytes written) when the handle times every launch.  max_err: P of `seq -q` (an integer 0 .. 10^9, None: off;
        cornetto_fqseq_set_max_err): `keep` of the records is then 1 for the printed ones, self.fq_qstats = [reads, bases printed] and
        self.fq_qsums = the records' sums of quality weights (uint64; None without max_err)."""
        L = self.L
        parts = data if isinstance(data, (list, tuple)) else [Bgzf(data) if bgzf_in else data]
        fq = None
        pins, cap = [None] * 4, [0] * 4
        out, texts = [], []
        self.fq_timing = []

        def result():
            st = (C.c_int64 * 5)()
            L.cornetto_fqseq_stats(fq, st)
            p, n = C.c_void_p(), C.c_int64()
            self._chk(L.cornetto_fqseq_records(self.h, fq, C.byref(p), C.byref(n)))
            ms, nb = C.c_double(), C.c_int64()
            self._chk(L.cornetto_fqseq_text_time(self.h, fq, C.byref(ms), C.byref(nb)))
            self.fq_text_time = (ms.value, nb.value)
            qs = (C.c_int64 * 2)()
            L.cornetto_fqseq_qstats(fq, qs)
            self.fq_qstats, self.fq_qsums = list(qs), None
            if max_err is not None:
                ps, ns = C.c_void_p(), C.c_int64()
                self._chk(L.cornetto_fqseq_qsums(self.h, fq, C.byref(ps), C.byref(ns)))
                self.fq_qsums = _take(L, ps, ns.value, np.dtype(np.uint64))
            return out if bgzf_out else b"".join(out), list(st)[:4], _take(L, p, n.value, FQREC_DT), int(L.cornetto_fqseq_rest(fq))

        def pull(n_text):
            pend, at, k = [0] * 4, 0, 0
            while at < n_text or any(pend):
                s = k & 3
                k += 1
                if pend[s]:
                    if bgzf_out:
                        nz = C.c_int64()
                        self._chk(L.cornetto_fqseq_wait_bgzf(self.h, fq, s, C.byref(nz)))
                        out.append(C.string_at(pins[s], nz.value))
                    else:
                        self._chk(L.cornetto_fqseq_wait(self.h, fq, s))
                        out.append(C.string_at(pins[s], pend[s]))
                    pend[s] = 0
                if at < n_text:
                    n = min(slab or n_text, n_text - at)
                    need = (n + 65279) // 65280 * 65536 if bgzf_out else n
                    if cap[s] < need:
                        if pins[s]:
                            L.cornetto_pinned_free(pins[s])
                        pins[s] = L.cornetto_pinned_alloc(need)
                        cap[s] = need
                        if not pins[s]:
                            raise MemoryError("cornetto_pinned_alloc(%d)" % need)
                    if bgzf_out:
                        self._chk(L.cornetto_fqseq_get_bgzf(self.h, fq, pins[s], cap[s], at, n, s))
                    else:
                        self._chk(L.cornetto_fqseq_get(self.h, fq, pins[s], at, n, s))
                    pend[s] = n
                    at += n

        def sources():
            """(BgSrc with what it points to, units in it, is it the stream's last) for every feed group"""
            groups = []
            for part in parts:
                if isinstance(part, Bgzf):
                    blocks, resume, broken = bgzf_scan(part.blob)
                    if broken or resume != len(part.blob):
                        raise ValueError("not a chain of BGZF members")
                    comp = self._text_from(part.blob)
                    texts.append(comp)
                    cuts = [len(blocks) * i // feeds for i in range(feeds + 1)]
                    groups += [("z", comp, np.ascontiguousarray(blocks[cuts[i]:cuts[i + 1]])) for i in range(feeds)]
                else:
                    t = bytes(part)
                    cuts = [len(t) * i // feeds for i in range(feeds + 1)]
                    groups += [("t", None, t[cuts[i]:cuts[i + 1]]) for i in range(feeds)]
            return groups
        try:
            opt = FqSeqOpt()
            L.cornetto_fqseq_defaults(C.byref(opt))
            opt.min_len, opt.records = min_len, 1
            if window is not None:
                opt.window = window
            fq = C.c_void_p()
            self._chk(L.cornetto_fqseq_open(self.h, C.byref(opt), C.byref(fq)))
            if max_err is not None:
                self._chk(L.cornetto_fqseq_set_max_err(self.h, fq, max_err))
            groups = sources()
            plain = True
            for gi, (kind, comp, body) in enumerate(groups):
                last = gi == len(groups) - 1
                at, n_all, first = 0, len(body), True
                while plain and (at < n_all or (first and last)):
                    first = False
                    if kind == "z":
                        keep = np.ascontiguousarray(body[at:])
                        src = BgSrc(None, 0, comp, keep.ctypes.data if keep.size else None, keep.size)
                    else:
                        keep = body[at:]
                        src = BgSrc(keep, len(keep), None, None, 0)
                    taken, n_text, pl = C.c_int64(), C.c_int64(), C.c_int32()
                    rc = L.cornetto_fqseq_feed(self.h, fq, C.byref(src), 1 if last else 0, C.byref(taken), C.byref(n_text), C.byref(pl))
                    self.fq_timing += self.last_timing()
                    if rc == -4:
                        try:
                            self._chk(rc)
                        except AccelError as e:
                            e.taken = taken.value
                            raise
                    if rc not in (0, -6):
                        self._chk(rc)
                    pull(n_text.value)
                    if rc == -6:
                        err = FastqBlockError(int(L.cornetto_fqseq_error(fq)))
                        err.text, err.stats, err.records, err.rest = result()
                        none = BgSrc(None, 0, None, None, 0)
                        err.refeed = L.cornetto_fqseq_feed(self.h, fq, C.byref(none), 1, C.byref(taken), C.byref(n_text), C.byref(pl))
                        raise err
                    at += taken.value
                    plain = bool(pl.value)
                if not plain:
                    break
            return result() + (plain,)
        finally:
            for p in pins:
                if p:
                    L.cornetto_pinned_free(p)
            if fq is not None and fq.value:
                L.cornetto_fqseq_close(self.h, fq)
            for t in texts:
                L.cornetto_text_free(self.h, t)

    def bedgraph_runs_ingest(self, tot_pieces, mq_pieces, alternate=True):
        """stream two RUN-LENGTH bedgraphs (iterables of bytes pieces, any split points) through cornetto_bgrun_*; returns what
        bedgraph_ingest() returns for their per-base expansion.  alternate: the pieces of the two files take turns (else all of cov-total,
        then all of cov-mq).  Raises BedgraphFormatError (kind, file, record, a, b of cornetto_bgrunerr_t)."""
        L = self.L
        bg = C.c_void_p()
        self._chk(L.cornetto_bgrun_open(self.h, C.byref(bg)))
        try:
            pieces = [list(tot_pieces) or [b""], list(mq_pieces) or [b""]]
            if alternate:
                order = sorted((i, f) for f in (0, 1) for i in range(len(pieces[f])))
            else:
                order = [(i, f) for f in (0, 1) for i in range(len(pieces[f]))]

            def check(rc):
                if rc == -6:
                    e = L.cornetto_bgrun_error(bg).contents
                    raise BedgraphFormatError(e.kind, e.record, e.a, e.b, e.file)
                self._chk(rc)
            for i, f in order:
                t = pieces[f][i]
                check(L.cornetto_bgrun_feed(self.h, bg, f, t, len(t), 1 if i == len(pieces[f]) - 1 else 0))
            cov, nc, names, ncl = C.c_void_p(), C.c_int32(), C.POINTER(C.c_char_p)(), C.c_int64()
            check(L.cornetto_bgrun_finish(self.h, bg, C.byref(cov), C.byref(nc), C.byref(names), C.byref(ncl)))
            return self._ingested(cov, nc, names, ncl)
        finally:
            L.cornetto_bgrun_close(self.h, bg)

    # ---- bedgraph ingest from sources (cornetto_bgsrc_t): plain pieces or the blocks of a BGZF blob ---------------------------------
    def _src_feeds(self, f, texts):
        """a depth file (a list of bytes pieces, or a Bgzf) -> its feeds: BgSrc structures with whatever they point to kept alive beside them"""
        if not isinstance(f, Bgzf):
            return [(BgSrc(p, len(p), None, None, 0), p) for p in (list(f) or [b""])]
        blocks, resume, broken = bgzf_scan(f.blob)
        if broken or resume != len(f.blob):
            raise ValueError("not a chain of BGZF members")
        comp = self._text_from(f.blob)
        texts.append(comp)
        out, at = [], 0
        for k in f.counts(len(blocks)):
            part = np.ascontiguousarray(blocks[at:at + k])
            at += k
            out.append((BgSrc(None, 0, comp, part.ctypes.data if k else None, k), part))
        return out

    def bedgraph_ingest_src(self, tot, mq, pending=None):
        """bedgraph_ingest() through cornetto_bgin_feed_src(): each of tot / mq is a list of bytes pieces (plain text) or a Bgzf (the file as a
        BGZF blob, inflated on the device); feed i takes piece / block group i of both.  pending: a list that receives
        cornetto_bgin_pending() after every feed.  Raises BedgraphFormatError (kind 11: a damaged block; file, record = its index).  The
        kernel times of all feeds are kept in self.bg_timing."""
        L = self.L
        bg, texts = C.c_void_p(), []
        self.bg_timing = []
        self._chk(L.cornetto_bgin_open(self.h, C.byref(bg)))
        try:
            ft, fq = self._src_feeds(tot, texts), self._src_feeds(mq, texts)
            n_t, n_q = len(ft), len(fq)
            nothing = (BgSrc(None, 0, None, None, 0), None)
            for i in range(max(n_t, n_q)):
                t, q = ft[i] if i < n_t else nothing, fq[i] if i < n_q else nothing
                fin = (1 if i >= n_t - 1 else 0) | (2 if i >= n_q - 1 else 0)
                rc = L.cornetto_bgin_feed_src(self.h, bg, C.byref(t[0]), C.byref(q[0]), fin)
                self.bg_timing += self.last_timing()
                if rc == -6:
                    e = L.cornetto_bgin_error(bg).contents
                    raise BedgraphFormatError(e.kind, e.record, e.a, e.b, e.file if e.kind == BG_BLOCK else None)
                self._chk(rc)
                if pending is not None:
                    a, b = C.c_int64(), C.c_int64()
                    L.cornetto_bgin_pending(bg, C.byref(a), C.byref(b))
                    pending.append((a.value, b.value))
                if L.cornetto_bgin_done(bg):
                    break
            cov, nc, names, ncl = C.c_void_p(), C.c_int32(), C.POINTER(C.c_char_p)(), C.c_int64()
            self._chk(L.cornetto_bgin_finish(self.h, bg, C.byref(cov), C.byref(nc), C.byref(names), C.byref(ncl)))
            return self._ingested(cov, nc, names, ncl)
        finally:
            L.cornetto_bgin_close(self.h, bg)
            for t in texts:
                L.cornetto_text_free(self.h, t)

    def bedgraph_runs_ingest_src(self, tot, mq, alternate=True):
        """bedgraph_runs_ingest() through cornetto_bgrun_feed_src(): each of tot / mq is a list of bytes pieces or a Bgzf"""
        L = self.L
        bg, texts = C.c_void_p(), []
        self.bg_timing = []
        self._chk(L.cornetto_bgrun_open(self.h, C.byref(bg)))
        try:
            feeds = [self._src_feeds(tot, texts), self._src_feeds(mq, texts)]
            if alternate:
                order = sorted((i, f) for f in (0, 1) for i in range(len(feeds[f])))
            else:
                order = [(i, f) for f in (0, 1) for i in range(len(feeds[f]))]

            def check(rc):
                if rc == -6:
                    e = L.cornetto_bgrun_error(bg).contents
                    raise BedgraphFormatError(e.kind, e.record, e.a, e.b, e.file)
                self._chk(rc)
            for i, f in order:
                rc = L.cornetto_bgrun_feed_src(self.h, bg, f, C.byref(feeds[f][i][0]), 1 if i == len(feeds[f]) - 1 else 0)
                self.bg_timing += self.last_timing()
                check(rc)
            cov, nc, names, ncl = C.c_void_p(), C.c_int32(), C.POINTER(C.c_char_p)(), C.c_int64()
            check(L.cornetto_bgrun_finish(self.h, bg, C.byref(cov), C.byref(nc), C.byref(names), C.byref(ncl)))
            return self._ingested(cov, nc, names, ncl)
        finally:
            L.cornetto_bgrun_close(self.h, bg)
            for t in texts:
                L.cornetto_text_free(self.h, t)

    def bedgraph_ingest(self, tot_pieces, mq_pieces, prefetch=0):
        """stream the two per-base bedgraphs (iterables of bytes pieces, any split points) through the device
        parser; returns (resident coverage, [contig names], clamped count).  Raises BedgraphFormatError.
        prefetch: 1 = cornetto_bgin_prefetch() of the next pieces in front of every feed (two pieces on their way, as the CLI does);
        2 = the same, and every third prefetch is of pieces that are NOT fed next (the feed must ignore what is staged)"""
        L = self.L
        bg = C.c_void_p()
        self._chk(L.cornetto_bgin_open(self.h, C.byref(bg)))
        try:
            ta, qa = list(tot_pieces), list(mq_pieces)
            n_t, n_q = len(ta), len(qa)
            n = max(n_t, n_q, 1)
            # (ctypes hands a bytes object's own buffer to a c_char_p parameter: the same address for the prefetch and the feed that follows)
            ta += [b""] * (n - n_t)
            qa += [b""] * (n - n_q)
            if prefetch:
                self._chk(L.cornetto_bgin_prefetch(self.h, bg, ta[0], len(ta[0]), qa[0], len(qa[0])))
            for i in range(n):
                t, q = ta[i], qa[i]
                fin = (1 if i >= n_t - 1 else 0) | (2 if i >= n_q - 1 else 0)
                if prefetch and i + 1 < n:
                    j = i + 1 if not (prefetch == 2 and i % 3 == 2) else 0          # (mode 2: something else than the next pieces now and then)
                    self._chk(L.cornetto_bgin_prefetch(self.h, bg, ta[j], len(ta[j]), qa[j], len(qa[j])))
                rc = L.cornetto_bgin_feed(self.h, bg, t, len(t), q, len(q), fin)
                if rc == -6:
                    e = L.cornetto_bgin_error(bg).contents
                    raise BedgraphFormatError(e.kind, e.record, e.a, e.b)
                self._chk(rc)
                if L.cornetto_bgin_done(bg):
                    break
            cov, nc, names, ncl = C.c_void_p(), C.c_int32(), C.POINTER(C.c_char_p)(), C.c_int64()
            self._chk(L.cornetto_bgin_finish(self.h, bg, C.byref(cov), C.byref(nc), C.byref(names), C.byref(ncl)))
            return self._ingested(cov, nc, names, ncl)
        finally:
            L.cornetto_bgin_close(self.h, bg)


def khash_str_order(names):
    """bucket order of the reference's khash string map after inserting `names` (list of bytes) in order:
    (slot per name, distinct ids in bucket order).  Host only."""
    L = lib()
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*names)
    slot = np.zeros(max(n, 1), np.int32)
    order = np.zeros(max(n, 1), np.int32)
    k = L.cornetto_khash_str_order(arr, n, slot.ctypes.data, order.ctypes.data)
    if k < 0:
        raise ValueError("cornetto_khash_str_order: bad argument")
    return slot[:n], order[:k]


class PanelOpt(C.Structure):
    _fields_ = [("min_lowq_len", C.c_int32), ("extend", C.c_int32), ("edge_len", C.c_int32), ("merge_dist", C.c_int32), ("min_ctg_len", C.c_int32),
                ("extend_right", C.c_int32), ("extend_gate", C.c_int32)]


def panel_boring(ctg_len, fun, lowq, recreate=False, **kw):
    """steps 4-9 of scripts/create-cornetto.sh (recreate=True: the constants of scripts/recreate-cornetto.sh) on index-based
    intervals (host only); kw overrides PanelOpt fields — `extend` alone sets all three of extend / extend_right / extend_gate"""
    L = lib()
    opt = PanelOpt()
    (L.cornetto_panel_defaults_recreate if recreate else L.cornetto_panel_defaults)(C.byref(opt))
    if "extend" in kw:
        kw.setdefault("extend_right", kw["extend"])
        kw.setdefault("extend_gate", kw["extend"])
    for k, v in kw.items():
        setattr(opt, k, v)
    ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
    fun = np.ascontiguousarray(fun, dtype=IVL_DT)
    lowq = np.ascontiguousarray(lowq, dtype=IVL_DT)
    p, n = C.c_void_p(), C.c_int64()
    rc = L.cornetto_panel_boring(ctg_len.ctypes.data, len(ctg_len), fun.ctypes.data, len(fun), lowq.ctypes.data, len(lowq), C.byref(opt), C.byref(p), C.byref(n))
    if rc != 0:
        raise ValueError("cornetto_panel_boring: status %d" % rc)
    return _take(L, p, n.value, IVL_DT)
