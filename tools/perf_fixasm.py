#!/usr/bin/env python3
"""development aid: `cornetto fixasm` on the bench's synthetic assembly (3.16 Gbp, 80-column or single-line), half of the contigs reversed
by a generated PAF.
   python tools/perf_fixasm.py --dir /dev/shm/fx --width 80 --reps 3        wall time of the CLI and of oracle/_ref/cornetto (alternating),
                                                                           stdout to /dev/null and to a file in --dir; sha256 of every output
   rocprofv3 --kernel-trace --stats -d OUT -- python tools/perf_fixasm.py --emit-only
                                                                           the emit kernel alone (cornetto_emit_* over the resident assembly,
                                                                           64 MiB windows): its time from the trace, bytes/s = 2 B per base;
                                                                           --serial: one window at a time (the kernel without copies beside it)"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref", "cornetto")


def assembly(torch, mbases):
    import bench
    dev = torch.device("cuda", 0)
    lens = bench.contig_lengths(int(mbases * 1e6))
    bases, offs = bench.make_assembly(torch, dev, lens, 0xC0FFEE)
    return bases, offs, lens


def emit_only(a):
    import torch
    import cornetto_amd
    bases, offs, lens = assembly(torch, a.mbases)
    acc = cornetto_amd.Accel(0)
    asm = acc.asm_wrap(bases.data_ptr(), offs, np.array(lens, dtype=np.int64))
    heads = b"".join(b">chr%d_%d\n" % (i % 24, i) for i in range(len(lens)))
    recs, h = [], 0
    for i in range(len(lens)):
        hl = len(b">chr%d_%d\n" % (i % 24, i))
        recs.append((i, i & 1, h, hl))
        h += hl
    L = acc.L
    r = np.array(recs, dtype=cornetto_amd.EMITREC_DT)
    hb = np.frombuffer(heads, dtype=np.uint8)
    S = a.slab << 20
    pins = [L.cornetto_pinned_alloc(S) for _ in range(4)]
    for rep in range(a.reps):
        e, total = C.c_void_p(), C.c_int64()
        t0 = time.perf_counter()
        acc._chk(L.cornetto_emit_open(acc.h, asm.ptr, r.ctypes.data, len(recs), hb.ctypes.data, len(heads), C.byref(e), C.byref(total)))
        nw = (total.value + S - 1) // S
        for w in range(nw):
            if w >= 4:
                acc._chk(L.cornetto_emit_wait(acc.h, e, w % 4))
            at = w * S
            acc._chk(L.cornetto_emit_get(acc.h, e, pins[w % 4], at, min(S, total.value - at), w % 4))
            if a.serial:      # (the kernel alone on the chip: the D2H blits of the other windows do not run beside it)
                acc._chk(L.cornetto_emit_wait(acc.h, e, w % 4))
        for s in range(4):
            acc._chk(L.cornetto_emit_wait(acc.h, e, s))
        dt = time.perf_counter() - t0
        L.cornetto_emit_free(acc.h, e)
        print("emit rep %d: %.1f MB of text in %d windows, %.1f ms incl. the copies to pinned memory = %.1f GB/s" %
              (rep, total.value / 1e6, nw, dt * 1e3, total.value / dt / 1e9), flush=True)
    for p in pins:
        L.cornetto_pinned_free(p)
    asm.close()
    acc.close()


def write_inputs(a, d):
    import torch
    bases, offs, lens = assembly(torch, a.mbases)
    hb = bases.cpu().numpy()
    fa = os.path.join(d, "asm%s.fa" % (a.width or "single"))
    with open(fa, "wb") as fh:
        for i, (o, L) in enumerate(zip(offs, lens)):
            s = hb[int(o):int(o) + int(L)]
            fh.write(b">ptg%06dl\n" % i)
            if a.width:
                k = len(s) // a.width * a.width
                m = np.empty((k // a.width, a.width + 1), dtype=np.uint8)
                m[:, :a.width] = s[:k].reshape(-1, a.width)
                m[:, a.width] = 10
                fh.write(m.tobytes())
                fh.write(s[k:].tobytes() + (b"\n" if len(s) > k else b""))
            else:
                fh.write(s.tobytes() + b"\n")
    paf = os.path.join(d, "asm.paf")
    with open(paf, "w") as fh:
        for i, L in enumerate(lens):
            fh.write("ptg%06dl\t%d\t0\t%d\t%s\tchr%d\t250000000\t0\t%d\t%d\t%d\t60\ttp:A:P\n" % (i, L, L, "+-"[i & 1], i % 24 + 1, L, L, L))
    del bases
    torch.cuda.empty_cache()
    return fa, paf, sum(int(x) for x in lens)


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--width", type=int, default=80, help="0 = one line per record")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/perf_fixasm")
    ap.add_argument("--slab", type=int, default=64, help="MiB per window (--emit-only)")
    ap.add_argument("--emit-only", action="store_true")
    ap.add_argument("--serial", action="store_true", help="--emit-only: every window's kernel and copy before the next window's")
    a = ap.parse_args()
    if a.emit_only:
        return emit_only(a)
    import cornetto_amd
    os.makedirs(a.dir, exist_ok=True)
    fa, paf, nb = write_inputs(a, a.dir)
    print("assembly: %.1f Mbases, %s; %d bytes of FASTA" % (nb / 1e6, "%d-column" % a.width if a.width else "single-line", os.path.getsize(fa)), flush=True)
    bins = [("ours", cornetto_amd.CLI_PATH)] + ([("ref", REF)] if os.path.exists(REF) else [])
    times = {}
    sums = {}
    for rep in range(a.reps):
        for name, b in bins:
            for dst in ("null", "file"):
                o = os.path.join(a.dir, "out_%s.fa" % name) if dst == "file" else os.devnull
                side = [os.path.join(a.dir, "%s_%s" % (name, x)) for x in ("r.tsv", "m.txt", "w.paf")]
                t0 = time.perf_counter()
                with open(o, "wb") as fo:
                    p = subprocess.run([b, "fixasm", "-r", side[0], "-m", side[1], "-w", side[2], fa, paf], stdout=fo, stderr=subprocess.PIPE)
                dt = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr.decode()[-2000:]
                times.setdefault((name, dst), []).append(dt)
                if dst == "file" and rep == a.reps - 1:
                    sums[name] = [sha(o)] + [sha(x) for x in side]
                    os.remove(o)
        print("rep %d: %s" % (rep, " ".join("%s/%s %.3f s" % (k[0], k[1], v[-1]) for k, v in times.items())), flush=True)
    for k, v in sorted(times.items()):
        print("%-5s stdout to %-4s: best %.3f s, median %.3f s (%.2f GB/s of output)" % (k[0], k[1], min(v), sorted(v)[len(v) // 2], nb / min(v) / 1e9))
    for name, s in sums.items():
        print("sha256 %-4s stdout %s  -r %s  -m %s  -w %s" % (name, s[0][:16], s[1][:16], s[2][:16], s[3][:16]))
    if len(sums) == 2:
        print("identical:", sums["ours"] == sums["ref"])


if __name__ == "__main__":
    main()
