"""ctypes binding of the cn_selftest_* entry points (cornetto_amd/csrc/selftest.hip, bgrun.hip): the scan primitives of wave.hpp /
scan.hpp / ivlmerge.hpp on their own, and the hook that sets the contents of a handle's workspaces (cn_selftest_ws_fill), in the DEVELOPMENT
build of the library only.  Not part of the C ABI; used by test_gpu_scan.py, test_gpu_ws_fill.py, test_ws_table.py and test_gpu_telofind_seams.py (the mark bitmap of the
telofind pass, cn_selftest_telo_marks).
Every function takes an `Accel(0, dev=True)` (the `dacc` fixture) and numpy arrays."""
import ctypes as C

import numpy as np

import cornetto_amd

WAVE_INCL_U32, WAVE_INCL_U64, WAVE_INCL_DPP, WAVE_SUM = 0, 1, 2, 3
E_ARG = -3

_bound = {}


def _lib():
    L = cornetto_amd.lib(dev=True)
    if id(L) in _bound:
        return L
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    sig = {
        "cn_selftest_wave": [vp, C.c_int, vp, vp, i64],
        "cn_selftest_block_excl": [vp, C.c_int, C.c_int, vp, vp, vp, i64],
        "cn_selftest_walk": [vp, vp, i64, i64, i64, u32, u32, C.POINTER(u32)],
        "cn_selftest_scan_u32": [vp, vp, i64, C.c_int, C.c_int, C.c_int, vp, vp],
        "cn_selftest_scan_set_epoch": [vp, u32],
        "cn_selftest_st_set_epoch": [vp, u32],
        "cn_selftest_merge_fused": [vp, vp, i64, i64, i32, vp, C.POINTER(i64)],
        "cn_selftest_scan_u64": [vp, vp, i64, C.POINTER(C.c_uint64)],
    }
    sig["cn_selftest_telo_marks"] = [vp, vp, C.c_char_p, vp, i64]
    sig["cn_selftest_ws_fill"] = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int]
    sig["cn_selftest_ws_class"] = [C.c_int, C.POINTER(C.c_char_p)]
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = args
    for name in ("cn_selftest_ws_name", "cn_selftest_pin_name"):
        fn = getattr(L, name)
        fn.restype = C.c_char_p
        fn.argtypes = [C.c_int]
    L.cn_selftest_sdust_core_handle.restype = vp
    L.cn_selftest_sdust_core_handle.argtypes = []
    _bound[id(L)] = True
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def wave(acc, which, v):
    """the wave primitive `which` over every 64 values of v (uint64 for WAVE_INCL_U64, else uint32)"""
    dt = np.uint64 if which == WAVE_INCL_U64 else np.uint32
    v = np.ascontiguousarray(v, dtype=dt)
    assert v.size % 64 == 0
    out = np.empty_like(v)
    acc._chk(_lib().cn_selftest_wave(acc.h, which, _p(v), _p(out), v.size))
    return out


def block_excl(acc, threads, v):
    """block_excl<T, threads> per `threads` values of v (uint32 or uint64): (prefixes, totals)"""
    assert v.dtype in (np.uint32, np.uint64) and v.size % threads == 0
    v = np.ascontiguousarray(v)
    pre, tot = np.empty_like(v), np.empty(v.size // threads, dtype=v.dtype)
    acc._chk(_lib().cn_selftest_block_excl(acc.h, threads, int(v.dtype == np.uint64), _p(v), _p(pre), _p(tot), v.size // threads))
    return pre, tot


def walk_rc(acc, words, stride, tile, epoch, own):
    """lookback_excl by one wave over `words` (uint64, updated in place; tile t's state is words[t * stride + stride - 1]):
    (status, excl)"""
    assert words.dtype == np.uint64 and words.flags.c_contiguous
    excl = C.c_uint32(0)
    rc = _lib().cn_selftest_walk(acc.h, _p(words), words.size, stride, tile, epoch, own, C.byref(excl))
    return rc, int(excl.value)


def scan_u32(acc, rec, n, stride, first, m, totals=True):
    """exclusive_u32_multi over counters first .. first + m - 1 of the n records of `stride` words in rec: (outs [m, n], totals [m] or None)"""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    assert rec.size == n * stride
    outs = np.empty((m, n), dtype=np.uint32)
    tot = np.zeros(m, dtype=np.uint64) if totals else None
    acc._chk(_lib().cn_selftest_scan_u32(acc.h, _p(rec), n, stride, first, m, _p(outs), _p(tot) if totals else None))
    return outs, tot


def scan_set_epoch(acc, epoch):
    acc._chk(_lib().cn_selftest_scan_set_epoch(acc.h, epoch))


def st_set_epoch(acc, epoch):
    acc._chk(_lib().cn_selftest_st_set_epoch(acc.h, epoch))


def merge_fused(acc, ivls, dist=0, n_cap=None):
    """cnivl::merge_fused over ivls (IVL_DT, ordered by contig and start)"""
    ivls = np.ascontiguousarray(ivls, dtype=cornetto_amd.IVL_DT)
    out = np.empty(ivls.size, dtype=cornetto_amd.IVL_DT)
    n = C.c_int64(0)
    acc._chk(_lib().cn_selftest_merge_fused(acc.h, _p(ivls), ivls.size, ivls.size if n_cap is None else n_cap, dist, _p(out), C.byref(n)))
    return out[:n.value]


WS_CLASSES = ("scratch", "vouched", "polled")


def _names(fn):
    out = []
    while fn(len(out)) is not None:
        out.append(fn(len(out)).decode())
    return out


def ws_names():
    """the device workspace slots by their enum names, in enum order (cn_selftest_ws_name)"""
    return _names(_lib().cn_selftest_ws_name)


def pin_names():
    return _names(_lib().cn_selftest_pin_name)


def ws_classes():
    """{slot name: (class of WS_CLASSES, the host fields that vouch for its contents or "")}: the hook's table (cn_selftest_ws_class)"""
    out = {}
    for i, name in enumerate(ws_names()):
        v = C.c_char_p()
        out[name] = (WS_CLASSES[_lib().cn_selftest_ws_class(i, C.byref(v))], v.value.decode())
    return out


def ws_fill_rc(acc, byte):
    """cn_selftest_ws_fill: every allocated workspace of the handle set to `byte` over its whole capacity, the vouchers of the vouched slots
    dropped, the polled slots (WS_SCAN, WS_STITCH) left alone -> (status, {name: bytes filled}, {name: bytes skipped}, {pinned name: bytes
    filled}), slots with 0 bytes left out.  BETWEEN COMPLETE OPERATIONS ONLY: E_ARG, nothing touched, while sdust_begin() waits for its
    sdust_end() or a lazy handle's copies are out; never while a bgin / bgrun session has a feed or a prefetch on its way or a text object's
    slabs are in flight (they use queues of their own: the handle cannot tell, and the hook waits for the handle's own streams only)."""
    dn, pn = ws_names(), pin_names()
    f, s, p = np.zeros(len(dn), np.int64), np.zeros(len(dn), np.int64), np.zeros(len(pn), np.int64)
    rc = _lib().cn_selftest_ws_fill(acc.h, byte, _p(f), _p(s), len(dn), _p(p), len(pn))
    if rc != 0:
        return rc, {}, {}, {}
    return (rc, {n: int(v) for n, v in zip(dn, f) if v}, {n: int(v) for n, v in zip(dn, s) if v}, {n: int(v) for n, v in zip(pn, p) if v})


class _Handle:
    """a handle the library owns, with what ws_fill() needs of an Accel"""

    def __init__(self, h):
        self.h = C.c_void_p(h)

    def _chk(self, rc):
        if rc != 0:
            raise cornetto_amd.AccelError(rc, _lib().cornetto_accel_last_error(self.h).decode())


def sdust_core_handle():
    """the process-wide handle of cornetto_sdust() / cornetto_sdust_core() in the development build; None before their first call"""
    h = _lib().cn_selftest_sdust_core_handle()
    return _Handle(h) if h else None


def ws_fill(acc, byte):
    rc, filled, skipped, pinned = ws_fill_rc(acc, byte)
    acc._chk(rc)
    return filled, skipped, pinned


def scan_u64(acc, v):
    """the 64-bit scan of bgrun.hip: (exclusive prefixes, total)"""
    io = np.array(v, dtype=np.uint64)
    tot = C.c_uint64(0)
    acc._chk(_lib().cn_selftest_scan_u64(acc.h, _p(io), io.size, C.byref(tot)))
    return io, int(tot.value)


def telo_marks(acc, asm, motif, n_words):
    """cn_telo_marks_impl over the resident assembly `asm` of this handle: the first n_words = sum of ceil(len / 64) words of the mark bitmap,
    the contigs back to back from multiples of 64 bits (uint64)"""
    out = np.empty(n_words, dtype=np.uint64)
    acc._chk(_lib().cn_selftest_telo_marks(acc.h, asm.ptr, motif, _p(out), n_words))
    return out
