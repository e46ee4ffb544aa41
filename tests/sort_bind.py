"""ctypes binding of cn_selftest_sort_pairs (cornetto_amd/csrc/selftest.hip): the radix sort of sort.hpp on its own, in the DEVELOPMENT build
of the library only.  Not part of the C ABI; used by test_gpu_hap.py with an `Accel(0, dev=True)` (the `dacc` fixture)."""
import ctypes as C

import numpy as np

import cornetto_amd

SO_TILE = 1024        # cnsort::SO_TILE: pairs per workgroup of a pass
SCAN_TILE = 4096      # cnscan::SC_TILE: counters per workgroup of the table's scan

_bound = {}


def _lib():
    L = cornetto_amd.lib(dev=True)
    if id(L) not in _bound:
        L.cn_selftest_sort_pairs.restype = C.c_int
        L.cn_selftest_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        _bound[id(L)] = True
    return L


def sort_pairs(acc, keys, vals, key_bits=64):
    """cnsort::pairs_u64 over (keys uint64, vals uint32) -> (sorted keys, their payloads)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    vals = np.ascontiguousarray(vals, dtype=np.uint32)
    assert keys.size == vals.size
    ok, ov = np.empty_like(keys), np.empty_like(vals)
    acc._chk(_lib().cn_selftest_sort_pairs(acc.h, keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), keys.size, key_bits,
                                           ok.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p)))
    return ok, ov
