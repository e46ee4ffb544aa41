#!/usr/bin/env python3
"""development aid: `cornetto noboringbits` on BGZF-compressed depth files (inflated on the device: cornetto_bgin_feed_src /
cornetto_bgrun_feed_src) against the same command on the plain files, and against the parent commit's binary (`_old/cornetto` beside
`_old/libcornetto_hip.so`) on the plain files, in alternating runs on one box.

The input is a synthetic per-base pair: 10 contigs, --mbp million positions in all (50: about 1 GB per file), depth piecewise constant with a
change every ~400 bases (what reads of 15 kb at 30x leave), two-digit values, the lines as `samtools depth -aa | awk` writes them
(name, pos, pos + 1, depth: no padding).  Each file is written plain and as BGZF in blocks of 65280 bytes (zlib level 6, what bgzip and
mosdepth write), and again as maximal runs for `--runs`.  Everything sits in the page cache (--dir on tmpfs, or read once before).
   python tools/perf_bgcomp.py --dir /dev/shm/bgcomp [--mbp 50] [--reps 5] [--old _old/cornetto] [--kernels] [--sweep]
prints: the stdout of every leg hashes equal; per leg the median and the range of the process wall time; with --kernels the event times of
bgzf_inflate / bgzf_crc32 over this text (GB/s of inflated bytes) and of the tokeniser and record kernels, from one ingest through the C ABI."""
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
BLOCK = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _bgzf(data):
    out = []
    for k in range(0, len(data), BLOCK):
        d = data[k:k + BLOCK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(p) + 25).to_bytes(2, "little") + p +
                   (zlib.crc32(d) & 0xFFFFFFFF).to_bytes(4, "little") + len(d).to_bytes(4, "little"))
    return b"".join(out)


def bgzf_file(src, dst, workers):
    """src -> dst in members of BLOCK bytes; the pieces are cut at multiples of BLOCK, so the chain is the one a single pass writes"""
    piece = BLOCK * 256
    with open(src, "rb") as f, open(dst, "wb") as o, ProcessPoolExecutor(workers) as ex:
        def pieces():
            while True:
                b = f.read(piece)
                if not b:
                    return
                yield b
        for part in ex.map(_bgzf, pieces()):
            o.write(part)
        o.write(EOF_BLOCK)


def per_base_rows(name, vals, lo, hi):
    """the lines of positions [lo, hi) — the same number of digits in pos and in pos + 1 over the whole range — as bytes"""
    w0, w1 = len(str(lo)), len(str(lo + 1))
    assert len(str(hi - 1)) == w0 and len(str(hi)) == w1
    n, ln = hi - lo, len(name)
    W = ln + 1 + w0 + 1 + w1 + 1 + 2 + 1
    out = np.empty((n, W), dtype=np.uint8)
    out[:, :ln] = np.frombuffer(name, dtype=np.uint8)
    p = np.arange(lo, hi, dtype=np.int64)

    def digits(v, col, nd):
        v = v.copy()
        for k in range(nd):
            out[:, col + nd - 1 - k] = v % 10 + 48
            v //= 10
    c = ln
    out[:, c] = 9
    digits(p, c + 1, w0)
    c += 1 + w0
    out[:, c] = 9
    digits(p + 1, c + 1, w1)
    c += 1 + w1
    out[:, c] = 9
    digits(vals[lo:hi].astype(np.int64), c + 1, 2)
    out[:, c + 3] = 10
    return out.tobytes()


def synthesize(a):
    os.makedirs(a.dir, exist_ok=True)
    names = {k: [os.path.join(a.dir, "m%d.%s.%s" % (a.mbp, k, f)) for f in ("total.bg", "mq20.bg")] for k in ("base", "runs")}
    names["base_z"] = [p + ".gz" for p in names["base"]]
    names["runs_z"] = [p + ".gz" for p in names["runs"]]
    if all(os.path.exists(p) for v in names.values() for p in v):
        return names
    rng = np.random.default_rng(0xC0FFEE)
    n_ctg, L = 10, a.mbp * 1_000_000 // 10
    edges = sorted({0, L} | {x for k in range(1, 12) for x in (10 ** k - 1, 10 ** k) if 0 < x < L})
    fh = {k: [open(p, "wb") for p in names[k]] for k in ("base", "runs")}
    for c in range(n_ctg):
        name = b"ptg%06dl" % (c + 1)
        n_seg = L // 400 + 2
        seg = np.minimum(np.cumsum(rng.geometric(1 / 400.0, n_seg)), L)
        seg = np.unique(np.concatenate([[0], seg, [L]]))
        depth = np.clip(35 + np.cumsum(rng.integers(-2, 3, len(seg) - 1)) % 40 - 10, 10, 99)
        for f, vals_seg in enumerate((depth, np.clip(depth - rng.integers(0, 6, len(depth)), 10, 99))):
            vals = np.repeat(vals_seg, np.diff(seg)).astype(np.uint8)
            for lo, hi in zip(edges[:-1], edges[1:]):
                for s in range(lo, hi, 1 << 22):
                    fh["base"][f].write(per_base_rows(name, vals, s, min(hi, s + (1 << 22))))
            first = np.flatnonzero(np.concatenate([[True], vals[1:] != vals[:-1]]))
            ends = np.concatenate([first[1:], [L]])
            fh["runs"][f].write(b"".join(b"%s\t%d\t%d\t%d\n" % (name, s, e, vals[s]) for s, e in zip(first.tolist(), ends.tolist())))
    for v in fh.values():
        for f in v:
            f.close()
    for k in ("base", "runs"):
        for src, dst in zip(names[k], names[k + "_z"]):
            bgzf_file(src, dst, a.workers)
    return names


def timed(argv, env):
    t0 = time.perf_counter()
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, (argv, p.stderr.decode()[-2000:])
    return dt, hashlib.sha256(p.stdout).hexdigest()


def kernels(a, names):
    """one ingest of the BGZF pair (and of the run pair) through the C ABI, 1024 blocks per feed: the sums of the event times per kernel"""
    import cornetto_amd
    from cornetto_amd import Bgzf
    acc = cornetto_amd.Accel(0)
    for kind, ingest in (("base_z", acc.bedgraph_ingest_src), ("runs_z", acc.bedgraph_runs_ingest_src)):
        blobs = [open(p, "rb").read() for p in names[kind]]
        text_bytes = sum(os.path.getsize(p) for p in names[kind[:-2]])
        for rep in range(2):              # (the first ingest loads the code objects and grows the work spaces)
            cov, nm, ncl = ingest(Bgzf(blobs[0], 1024), Bgzf(blobs[1], 1024))
            cov.close()
        tot = {}
        for k, ms in acc.bg_timing:
            tot[k] = tot.get(k, 0.0) + ms
        print("kernels, %s: %.1f MB compressed -> %.1f MB of text, %d launches" % (kind, sum(len(b) for b in blobs) / 1e6, text_bytes / 1e6, len(acc.bg_timing)))
        for k, ms in sorted(tot.items(), key=lambda kv: -kv[1]):
            print("   %-14s %9.3f ms  %7.1f GB/s of text" % (k, ms, text_bytes / ms / 1e6))
    acc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--mbp", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old", default=os.path.join(ROOT, "_old", "cornetto"))
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="leg (a) again over $CORNETTO_BG_PIECE = 16 .. 1024 MB")
    ap.add_argument("--accel", default="yes", help="no: a rehearsal of the script on the host path")
    a = ap.parse_args()
    import cornetto_amd
    names = synthesize(a)
    for k, v in names.items():
        print("%-7s %s" % (k, "  ".join("%s %.1f MB" % (os.path.basename(p), os.path.getsize(p) / 1e6) for p in v)), flush=True)
    env = dict(os.environ)
    for k in ("CORNETTO_ACCEL", "CORNETTO_BGZF", "CORNETTO_BG_PIECE", "CORNETTO_DEVICES"):
        env.pop(k, None)
    new, old = cornetto_amd.CLI_PATH, a.old if os.path.exists(a.old) else None
    if not old:
        print("no %s: leg (c), the parent commit's binary on the plain pair, is left out" % a.old)
    opts = ["--accel=" + a.accel]
    for extra, plain, comp in (([], "base", "base_z"), (["--runs"], "runs", "runs_z")):
        legs = [("(a) this build, BGZF", [new, "noboringbits"] + extra + opts + [names[comp][0], "-q", names[comp][1]]),
                ("(b) this build, plain", [new, "noboringbits"] + extra + opts + [names[plain][0], "-q", names[plain][1]])]
        if old:
            legs.append(("(c) parent, plain", [old, "noboringbits"] + extra + opts + [names[plain][0], "-q", names[plain][1]]))
        times, hashes = {}, {}
        for rep in range(a.reps + 1):            # (the first round warms the page cache and the code objects: not counted)
            # every round begins with another leg: on runs of a fifth of a second the leg that follows a pause was 0.1 s slower than the one
            # behind it, whichever binary it was
            for name, argv in legs[rep % len(legs):] + legs[:rep % len(legs)]:
                dt, hx = timed(argv, env)
                hashes[name] = hx
                if rep:
                    times.setdefault(name, []).append(dt)
        assert len(set(hashes.values())) == 1, hashes
        print("%s: stdout sha256 %s on every leg" % (" ".join(extra) or "per base", hx[:16]))
        for name, v in times.items():
            print("   %-22s median %.3f s  (%.3f .. %.3f, %d runs)" % (name, sorted(v)[len(v) // 2], min(v), max(v), len(v)), flush=True)
        if a.sweep:
            # the inflated bytes per round: a wave inflates a block, so a round of 64 MB is a launch of about a thousand waves
            for mb in (16, 64, 256, 1024):
                v = sorted(timed(legs[0][1], dict(env, CORNETTO_BG_PIECE=str(mb << 20)))[0] for _ in range(3))
                print("   (a) with rounds of %4d MB: median %.3f s  (%.3f .. %.3f, 3 runs)" % (mb, v[1], v[0], v[2]), flush=True)
    if a.kernels:
        kernels(a, names)


if __name__ == "__main__":
    main()
