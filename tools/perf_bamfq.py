#!/usr/bin/env python3
"""development aid: `seq --bam` on a synthetic unaligned BAM of long reads — --mb million bytes of records, reads of about --read bases with
bases and qualities drawn at random (they do not compress: the decoder's worst case; the qualities of three reads in ten
are halved, so that `-q 10` drops a visible share), a dx:i:1 tag on a share of them,
half of them on the reverse strand, BGZF blocks of 65280 bytes (zlib level 1) — on the device and under --accel=no, against `seq -m N` on the
FASTQ text of the same reads (written here too: what a user has today once something else has made the text), with the parent commit's
binary (`_old/cornetto` beside `_old/libcornetto_hip.so`) when it is there and this build's otherwise — the code of that path is the same.
   python tools/perf_bamfq.py --dir /tmp/bamfq [--mb 500] [--runs 5] [--old _old/cornetto] [--kernels] [--sweep 64,256,1024]
prints: the stdout of the commands is the same; wall times of the process, alternating runs, files in the page cache; then `seq --bam` on the device
without and with -q 10, alternating, with --accel=no -q 10 and this build's seq -q 10 on the FASTQ text, whose text must be the same; with --kernels
the event times of one pass through the binding (bgzf_inflate, bgzf_crc32, bam_frame, bamfq_size, bamfq_scan, bamfq_text) without and with the filter,
and qmean_sum's time over the bytes of its windows and over the quality bytes it sums; with --sweep the wall time over
$CORNETTO_BAM_WINDOW (MiB).  `samtools fastq` is timed if it is on the box; nothing depends on it."""
import argparse
import os
import shutil
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
CODES = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
COMP = np.frombuffer(b"=TGKCYSBAWRDMHVN", dtype=np.uint8)


def _bgzf(data):
    out = []
    for k in range(0, len(data), BLOCK):
        d = data[k:k + BLOCK]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(p) + 25).to_bytes(2, "little") + p +
                   (zlib.crc32(d) & 0xFFFFFFFF).to_bytes(4, "little") + len(d).to_bytes(4, "little"))
    return b"".join(out)


def synthesize(d, mb, read_len, duplex_share, seed):
    """-> (BAM path, FASTQ path of all reads, FASTQ path of the dx:1 reads)"""
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, "reads.%s" % x) for x in ("bam", "fastq", "duplex.fastq")]
    if all(os.path.exists(p) for p in paths):
        return paths
    rng = np.random.default_rng(seed)
    low = np.random.default_rng(seed + 1)          # (a generator of its own: lengths, bases and tags are those of the files without -q)
    parts, n_reads, n_bytes = [b"BAM\1" + struct.pack("<ii", 0, 0)], 0, 0
    with open(paths[1], "wb") as f_all, open(paths[2], "wb") as f_dx:
        while n_bytes < mb * 1_000_000:
            l_seq = int(max(200, rng.normal(read_len, read_len / 3)))
            nib = (1 << rng.integers(0, 4, l_seq + (l_seq & 1))).astype(np.uint8)
            qual = rng.integers(0, 51, l_seq).astype(np.uint8)          # a mean error of 0.095: above Q10; halved, 0.18: below it
            if low.random() < 0.3:
                qual >>= 1
            rev = bool(rng.random() < 0.5)
            dx = bool(rng.random() < duplex_share)
            name = b"%08x-4c1d-4f7a-9c3e-%012d" % (n_reads * 2654435761 & 0xFFFFFFFF, n_reads)
            aux = b"qsi" + struct.pack("<i", 20) + b"mvBc" + struct.pack("<I", 32) + bytes(32) + b"RGZrun_1\0" + b"dxi" + struct.pack("<i", 1 if dx else 0)
            body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, 0, 4 | (16 if rev else 0), l_seq, -1, -1, 0) + name + b"\0" + \
                ((nib[0::2] << 4) | nib[1::2]).tobytes() + qual.tobytes() + aux
            parts.append(struct.pack("<i", len(body)) + body)
            n_bytes += len(body) + 4
            n_reads += 1
            codes = nib[:l_seq]
            text = b"@" + name + b"\n" + (COMP[codes[::-1]] if rev else CODES[codes]).tobytes() + b"\n+\n" + ((qual[::-1] if rev else qual) + 33).tobytes() + b"\n"
            f_all.write(text)
            if dx:
                f_dx.write(text)
    raw = b"".join(parts)
    del parts
    with ProcessPoolExecutor(16) as ex:
        step = BLOCK * 256
        blob = b"".join(ex.map(_bgzf, [raw[k:k + step] for k in range(0, len(raw), step)])) + EOF_BLOCK
    with open(paths[0], "wb") as f:
        f.write(blob)
    print("%d reads, %.0f MB of BAM records in %.0f MB of BGZF; FASTQ text %.0f MB, of the dx:1 reads %.0f MB" % (
        n_reads, len(raw) / 1e6, len(blob) / 1e6, os.path.getsize(paths[1]) / 1e6, os.path.getsize(paths[2]) / 1e6), flush=True)
    return paths


def wall(argv, env=None):
    """the process's wall time with its stdout sent to a pipe that a thread of this process empties -> (seconds, bytes, CRC-32 of stdout)"""
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    p = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    n, crc = 0, 0
    while True:
        piece = p.stdout.read(1 << 24)
        if not piece:
            break
        n += len(piece)
        crc = zlib.crc32(piece, crc)
    err = p.stderr.read()
    rc = p.wait()
    dt = time.perf_counter() - t0
    if rc != 0:
        raise SystemExit("%s failed (%d): %s" % (argv, rc, err.decode(errors="replace")[-2000:]))
    return dt, n, crc


def stats(xs):
    xs = sorted(xs)
    return "%.3f s (%.3f-%.3f)" % (xs[len(xs) // 2], xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--mb", type=int, default=500)
    ap.add_argument("--read", type=int, default=20000)
    ap.add_argument("--min-len", type=int, default=15000)
    ap.add_argument("--duplex-share", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old", default=os.path.join(ROOT, "_old", "cornetto"))
    ap.add_argument("--sweep", default="")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import cornetto_amd
    new = cornetto_amd.CLI_PATH
    text_bin = a.old if os.path.exists(a.old) else new
    print("the text path runs %s" % ("the parent commit's binary" if text_bin == a.old else "this build's seq (no parent binary at %s): the same code" % a.old), flush=True)
    bam, fastq, fastq_dx = synthesize(a.dir, a.mb, a.read, a.duplex_share, 21)
    m = str(a.min_len)
    for label, extra, text in (("all reads", [], fastq), ("--duplex", ["--duplex"], fastq_dx)):
        cmds = {"seq --bam, device": [new, "seq", "-m", m, "--bam", bam] + extra, "seq --bam, --accel=no": [new, "seq", "-m", m, "--accel=no", "--bam", bam] + extra,
                "seq on the FASTQ text": [text_bin, "seq", "-m", m, text]}
        if shutil.which("samtools") and not extra:
            cmds["samtools fastq"] = ["samtools", "fastq", bam]
        for argv in cmds.values():          # (one run of each unmeasured: the files are in the page cache afterwards)
            wall(argv)
        times, outs = {k: [] for k in cmds}, {}
        for _ in range(a.runs):
            for k, argv in cmds.items():
                dt, n, crc = wall(argv)
                times[k].append(dt)
                outs[k] = (n, crc)
        ours = [outs[k] for k in cmds if k != "samtools fastq"]
        print("%s, -m %s: stdout %s (%d bytes)" % (label, m, "the same" if len(set(ours)) == 1 else "DIFFERS %r" % (outs,), ours[0][0]), flush=True)
        for k in cmds:
            print("  %-24s %s" % (k, stats(times[k])), flush=True)
    # -q 10 beside the same command without it, alternating
    pairs = {"seq --bam, device": [new, "seq", "-m", m, "--bam", bam], "seq --bam, --accel=no": [new, "seq", "-m", m, "--accel=no", "--bam", bam],
             "seq on the FASTQ text (this build)": [new, "seq", "-m", m, fastq]}
    tq, outq = {(k, q): [] for k in pairs for q in (0, 1)}, {}
    for i in range(a.runs + 1):          # (the first round unmeasured)
        for k, argv in pairs.items():
            for q in (0, 1):
                dt, n, crc = wall(argv + (["-q", "10"] if q else []))
                if i:
                    tq[(k, q)].append(dt)
                outq[(k, q)] = (n, crc)
    same = len(set(outq[(k, 1)] for k in pairs)) == 1
    print("-m %s -q 10: stdout %s (%d of %d bytes)" % (m, "the same from all three" if same else "DIFFERS %r" % (outq,), outq[("seq --bam, device", 1)][0], outq[("seq --bam, device", 0)][0]), flush=True)
    for k in pairs:
        print("  %-36s %s   with -q 10: %s" % (k, stats(tq[(k, 0)]), stats(tq[(k, 1)])), flush=True)
    for mib in [int(x) for x in a.sweep.split(",") if x]:
        ts = [wall([new, "seq", "-m", m, "--bam", bam], {"CORNETTO_BAM_WINDOW": str(mib << 20)})[0] for _ in range(3)]
        print("window %4d MiB: %s" % (mib, stats(ts)), flush=True)
    if a.kernels:
        acc = cornetto_amd.Accel(0)
        with open(bam, "rb") as f:
            blob = f.read()
        for max_err in (None, 10 ** 8):
            for rep in range(2):
                text, st, _ = acc.bam_fastq(blob, a.min_len, False, window=256 << 20, slab=32 << 20, max_err=max_err)
            tm = {}
            for name, ms in acc.bam_timing:
                tm.setdefault(name, []).append(ms)
            print("kernels of one pass%s (window 256 MiB, slabs of 32 MiB, %d bytes of text): %s" % (
                "" if max_err is None else " with -q 10", len(text), "; ".join("%s %d x, %.2f ms in all, %.2f ms the longest" % (k, len(v), sum(v), max(v)) for k, v in tm.items())), flush=True)
            if max_err is not None:
                ms, n_win = sum(tm.get("qmean_sum", [0.0])), a.mb * 1_000_000
                print("qmean_sum: %d x, %.3f ms over windows of about %d bytes in all: %.0f GB/s of window, %.0f GB/s of the %d quality bytes it sums; %d of %d reads >= %d printed" % (
                    len(tm.get("qmean_sum", [])), ms, n_win, n_win / ms / 1e6 if ms > 0 else 0, st[3] / ms / 1e6 if ms > 0 else 0, st[3], acc.bam_qstats[0], st[2], a.min_len), flush=True)
        acc.close()


if __name__ == "__main__":
    main()
