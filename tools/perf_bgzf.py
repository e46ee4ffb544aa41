#!/usr/bin/env python3
"""development aid: `cornetto sdust` / `cornetto telofind` on the bench's synthetic 3.16 Gbp assembly written as BGZF (Python's zlib, 65280
bytes a block, level 6) — this tree's binary (blocks inflated on the device) alternating with the parent commit's binary (`_old/cornetto`
beside `_old/libcornetto_hip.so`: gzread on one host thread) and with the uncompressed file, at least 5 runs each; and the two kernels alone
under the profiler.
   python tools/perf_bgzf.py --dir /tmp/bgzf [--runs 5] [--old _old/cornetto]      the timing leg (one trace run at the end)
   rocprofv3 --kernel-trace --stats -d /tmp/bgzf/prof -- python tools/perf_bgzf.py --dir /tmp/bgzf --kernels
The files are written once and kept in --dir (--clean removes them)."""
import argparse
import hashlib
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


def _bgzf_chunk(args):
    path, at, n = args
    with open(path, "rb") as f:
        f.seek(at)
        data = f.read(n)
    out = []
    for k in range(0, len(data), BLOCK):
        d = data[k:k + BLOCK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(p) + 25).to_bytes(2, "little") + p +
                   (zlib.crc32(d) & 0xFFFFFFFF).to_bytes(4, "little") + len(d).to_bytes(4, "little"))
    return b"".join(out)


def write_files(d):
    fa, bz = os.path.join(d, "asm80.fa"), os.path.join(d, "asm80.fa.gz")
    if os.path.exists(fa) and os.path.exists(bz):
        return fa, bz
    import torch
    import bench
    dev = torch.device("cuda", 0)
    lens = bench.contig_lengths(0)
    bases, offs = bench.make_assembly(torch, dev, lens, 0xC0FFEE)
    hb = bases.cpu().numpy()
    del bases
    torch.cuda.empty_cache()
    with open(fa, "wb") as f:
        for i, (o, L) in enumerate(zip(offs, lens)):
            f.write(b">ptg%06dl\n" % i)
            a = hb[int(o):int(o) + int(L)]
            k = len(a) // 80 * 80
            m = np.empty((k // 80, 81), dtype=np.uint8)
            m[:, :80] = a[:k].reshape(-1, 80)
            m[:, 80] = 10
            f.write(memoryview(m.reshape(-1)))
            f.write(memoryview(a[k:]))
            f.write(b"\n")
    size = os.path.getsize(fa)
    step = BLOCK * 256
    t0 = time.perf_counter()
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex, open(bz, "wb") as f:
        for part in ex.map(_bgzf_chunk, [(fa, at, step) for at in range(0, size, step)], chunksize=4):
            f.write(part)
        f.write(EOF_BLOCK)
    print("wrote %s (%d bytes) and %s (%d bytes, %.1f s of zlib on the host)" % (fa, size, bz, os.path.getsize(bz), time.perf_counter() - t0), flush=True)
    return fa, bz


def timing(a, fa, bz):
    import cornetto_amd
    new, old = cornetto_amd.CLI_PATH, os.path.join(ROOT, a.old)
    legs = [("new bgzf", new, bz, {}), ("old bgzf", old, bz, {}), ("new plain", new, fa, {})]
    if not os.path.exists(old):
        print("no %s: this tree's binary with CORNETTO_BGZF=0 (the parent's path) stands in for the parent commit's" % old)
        legs[1] = ("new bgzf, CORNETTO_BGZF=0", new, bz, {"CORNETTO_BGZF": "0"})
    for sub in ("sdust", "telofind"):
        times, outs = {k: [] for k, *_ in legs}, set()
        for r in range(a.runs):
            for name, exe, path, env in legs:         # alternating: one run of every leg per round
                t0 = time.perf_counter()
                p = subprocess.run([exe, sub, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env))
                times[name].append(time.perf_counter() - t0)
                outs.add((p.returncode, hashlib.md5(p.stdout).hexdigest()[:8]))
        for name, *_ in legs:
            t = sorted(times[name])
            print("%-9s %-26s median %.3f s  min %.3f  max %.3f  (%s)" % (sub, name, t[len(t) // 2], t[0], t[-1], " ".join("%.3f" % x for x in times[name])), flush=True)
        print("%-9s distinct (exit status, stdout) over all runs: %d" % (sub, len(outs)), flush=True)
    p = subprocess.run([new, "sdust", bz], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, CORNETTO_CLI_TRACE="1"))
    print(p.stderr.decode(errors="replace"))


def kernels(bz):
    """one cornetto_text_inflate() of the file in this process: for `rocprofv3 --kernel-trace --stats`, and the event times of the two kernels"""
    import ctypes as C
    import cornetto_amd
    acc = cornetto_amd.Accel(0)
    data = np.fromfile(bz, dtype=np.uint8)
    blocks, resume, broken = cornetto_amd.bgzf_scan(data)
    assert resume == data.size and not broken
    total = int(blocks["n_dst"].sum())
    comp, out, bad = acc._text_from(data), C.c_void_p(), C.c_int64()
    acc._chk(acc.L.cornetto_text_open(acc.h, total, C.byref(out)))
    for it in range(3):
        acc._chk(acc.L.cornetto_text_inflate(acc.h, comp, out, blocks.ctypes.data, blocks.size, C.byref(bad)))
        print("blocks %d, %.3f GB -> %.3f GB:" % (blocks.size, data.size / 1e9, total / 1e9),
              "  ".join("%s %.2f ms (%.0f GB/s of output)" % (n, ms, total / ms / 1e6) for n, ms in acc.last_timing()), flush=True)
    acc.L.cornetto_text_free(acc.h, comp)
    acc.L.cornetto_text_free(acc.h, out)
    acc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old", default="_old/cornetto")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    fa, bz = write_files(a.dir)
    if a.kernels:
        kernels(bz)
    else:
        timing(a, fa, bz)
    if a.clean:
        os.remove(fa)
        os.remove(bz)


if __name__ == "__main__":
    main()
