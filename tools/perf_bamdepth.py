#!/usr/bin/env python3
"""development aid: `noboringbits --bam` on a synthetic long-read BAM — 15 kb reads at 30x over an assembly of --mbp million bases, with
sequence and quality bytes, BGZF blocks of 65280 bytes (zlib level 1) — against the parent commit's binary (`_old/cornetto` beside
`_old/libcornetto_hip.so`) on the per-base bedgraph text of the same coverage (written here too: what the two `samtools depth -aa | awk`
passes of the protocol leave on the disk; their time is not in the text path's figure).  Two variants: `indel` (an insertion or a deletion
every ~25 bases) and `clean` (one every ~2000).
   python tools/perf_bamdepth.py --dir /tmp/bamdepth [--mbp 20] [--runs 5] [--old _old/cornetto]
prints: the stdout of the two commands is the same; wall times, alternating; the kernel times of one pass per window (event pairs:
bgzf_inflate, bgzf_crc32, bam_frame, bam_depth, bam_scan); the wall time over a sweep of $CORNETTO_BAM_WINDOW."""
import argparse
import os
import struct
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
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(p) + 25).to_bytes(2, "little") + p +
                   (zlib.crc32(d) & 0xFFFFFFFF).to_bytes(4, "little") + len(d).to_bytes(4, "little"))
    return b"".join(out)


def synthesize(d, tag, mbp, depth, read_len, indel_every, seed):
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, "%s.%s" % (tag, x)) for x in ("bam", "total.bg", "mq.bg")]
    if all(os.path.exists(p) for p in paths):
        return paths
    rng = np.random.default_rng(seed)
    n_ctg = 10
    ctg_len = mbp * 1_000_000 // n_ctg
    names = ["ptg%06dl" % i for i in range(n_ctg)]
    head = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", n_ctg)
    for nm in names:
        head += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ctg_len)
    pool = rng.integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
    diff = np.zeros((2, n_ctg, ctg_len + 1), dtype=np.int32)
    n_reads = mbp * 1_000_000 * depth // read_len
    parts, n_ops_all = [head], 0
    for i in range(n_reads):
        c = int(rng.integers(n_ctg))
        pos = int(rng.integers(0, ctg_len - read_len // 2))
        n_m = max(1, read_len // indel_every)
        m = rng.geometric(1.0 / indel_every, n_m).astype(np.int64)
        gap = rng.integers(1, 4, n_m).astype(np.int64)
        is_del = rng.random(n_m) < 0.5
        ops = np.empty(2 * n_m + 1, dtype=np.uint32)
        ops[0] = (20 << 4) | 4
        ops[1::2] = (m << 4).astype(np.uint32)
        ops[2::2] = ((gap << 4) | np.where(is_del, 2, 1)).astype(np.uint32)
        ops = ops[:-1]          # ends with an M
        adv = np.where(is_del, gap, 0)
        st = pos + np.concatenate(([0], np.cumsum(m + adv)[:-1]))
        en = np.minimum(st + m, ctg_len)
        st = np.minimum(st, ctg_len)
        mapq = 60 if rng.random() < 0.85 else int(rng.integers(0, 20))
        for q in range(2 if mapq >= 20 else 1):
            np.add.at(diff[q, c], st, 1)
            np.add.at(diff[q, c], en, -1)
        l_seq = int(20 + m.sum() + np.where(is_del, 0, gap)[:-1].sum())
        at = int(rng.integers(0, len(pool) - 2 * l_seq))
        body = struct.pack("<iiBBHHHIiii", c, pos, 9, mapq, 4680, len(ops), 0 if rng.random() < 0.5 else 16, l_seq, -1, -1, 0) + b"read%04d\0" % (i % 10000) + \
            ops.tobytes() + pool[at:at + (l_seq + 1) // 2] + pool[at + l_seq:at + 2 * l_seq] + b"NMC\5"
        parts.append(struct.pack("<i", len(body)) + body)
        n_ops_all += len(ops)
    raw = b"".join(parts)
    del parts
    with ProcessPoolExecutor(16) as ex:
        step = BLOCK * 256
        blob = b"".join(ex.map(_bgzf, [raw[k:k + step] for k in range(0, len(raw), step)])) + EOF_BLOCK
        with open(paths[0], "wb") as f:
            f.write(blob)
        for q in range(2):
            dep = np.cumsum(diff[q, :, :-1], axis=1)
            texts = ex.map(_bedgraph_at, [(names[c], dep[c, k:k + 500_000], k) for c in range(n_ctg) for k in range(0, ctg_len, 500_000)])
            with open(paths[1 + q], "wb") as f:
                for t in texts:
                    f.write(t)
    print("%s: %d reads, %.1f ops a read, %.0f MB of BAM records in %.0f MB of BGZF; bedgraphs %.0f + %.0f MB" % (
        tag, n_reads, n_ops_all / n_reads, len(raw) / 1e6, len(blob) / 1e6, os.path.getsize(paths[1]) / 1e6, os.path.getsize(paths[2]) / 1e6), flush=True)
    return paths


def _bedgraph_at(args):
    name, depth, base = args
    return "".join("%s\t%d\t%d\t%d\n" % (name, base + i, base + i + 1, v) for i, v in enumerate(depth.tolist())).encode()


def wall(argv, env=None):
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (argv, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    return dt, p.stdout


def stats(xs):
    xs = sorted(xs)
    return "%.3f s (%.3f-%.3f)" % (xs[len(xs) // 2], xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--mbp", type=int, default=20)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--read", type=int, default=15000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old", default=os.path.join(ROOT, "_old", "cornetto"))
    ap.add_argument("--sweep", default="32,64,128,256,512,1024")
    ap.add_argument("--variants", default="indel,clean")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    import cornetto_amd
    new = cornetto_amd.CLI_PATH
    for tag in a.variants.split(","):
        bam, tot, mq = synthesize(a.dir, tag, a.mbp, a.depth, a.read, 25 if tag == "indel" else 2000, 11 if tag == "indel" else 12)
        t_new, t_old = [], []
        wall([new, "noboringbits", "--bam", bam])           # (one run of each unmeasured: the files are in the page cache afterwards)
        wall([a.old, "noboringbits", "-q", mq, tot])
        for _ in range(a.runs):
            dt, out_new = wall([new, "noboringbits", "--bam", bam])
            t_new.append(dt)
            dt, out_old = wall([a.old, "noboringbits", "-q", mq, tot])
            t_old.append(dt)
        print("%s: stdout %s (%d bytes); --bam %s; parent binary on the bedgraph text %s" % (
            tag, "the same" if out_new == out_old else "DIFFERS", len(out_new), stats(t_new), stats(t_old)), flush=True)
        for mib in [int(x) for x in a.sweep.split(",")]:
            ts = [wall([new, "noboringbits", "--bam", bam], {"CORNETTO_BAM_WINDOW": str(mib << 20)})[0] for _ in range(3)]
            print("%s: window %4d MiB: %s" % (tag, mib, stats(ts)), flush=True)
        acc = cornetto_amd.Accel(0)
        with open(bam, "rb") as f:
            blob = f.read()
        window = 64 << 20
        n_blocks = len(blob) // 40000 + 1
        for rep in range(2):
            cov = acc.bam_depth(blob, window=window, feeds=max(1, n_blocks * BLOCK // window + 1))[0]
            cov.close()
        tm = {}
        for name, ms in acc.bam_timing:
            tm.setdefault(name, []).append(ms)
        print("%s: kernels of one pass, window 64 MiB: %s" % (tag, "; ".join("%s %d x, %.2f ms in all, %.2f ms the longest" % (k, len(v), sum(v), max(v)) for k, v in tm.items())),
              flush=True)
        acc.close()


if __name__ == "__main__":
    main()
