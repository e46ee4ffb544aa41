#!/usr/bin/env python3
"""development aid: `seq --fastq` on the synthetic long reads of tools/perf_bamfq.py as FASTQ text — --mb million bytes of text, reads of about
--read bases with bases and qualities drawn at random (they do not compress: the decoder's worst case; the qualities of three reads in ten
are halved, so that `-q 10` drops a visible share) — plain and bgzip-compressed (BGZF
blocks of 65280 bytes, zlib level 1), against the parent commit's `seq -m N` on the same two files (`_old/cornetto` beside
`_old/libcornetto_hip.so`; without it this build's positional `seq`, which is the same host code, and the output says so).
   python tools/perf_fqseq.py --dir /tmp/fqseq [--mb 500] [--runs 3] [--old _old/cornetto] [--kernels]
prints: whether the stdout of the commands is the same; wall times of the process, alternating runs, files in the page cache, stdout into
a pipe that this process empties: the parent's seq on the plain and on the .gz file, this build's --fastq plain -> plain, gz -> plain,
gz -> --bgzf, and --accel=no --fastq gz --bgzf; then the -q 10 legs beside their twins without -q, alternating on the same files: --fastq plain
and gz on the device, and this build's positional seq -q 10 (the host loop: the parent has no -q), whose text must be the same.  With --kernels:
the event times of one pass through the binding over the .gz file without and with the filter, fqseq_text's bytes read plus bytes written over
its time, and qmean_sum's time over the bytes of its windows and over the quality bytes it sums.  Never imported by the tests or by bench.py."""
import argparse
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
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bgzf(data):
    out = []
    for k in range(0, len(data), BLOCK):
        d = data[k:k + BLOCK]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(p) + 25).to_bytes(2, "little") + p +
                   (zlib.crc32(d) & 0xFFFFFFFF).to_bytes(4, "little") + len(d).to_bytes(4, "little"))
    return b"".join(out)


def synthesize(d, mb, read_len, seed):
    """-> (plain FASTQ path, BGZF path)"""
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, "reads-%d.%s" % (mb, x)) for x in ("fastq", "fastq.gz")]
    if all(os.path.exists(p) for p in paths):
        return paths
    rng = np.random.default_rng(seed)
    low = np.random.default_rng(seed + 1)          # (a generator of its own: lengths and bases are those of the files without -q)
    parts, n_reads, n_bytes = [], 0, 0
    while n_bytes < mb * 1_000_000:
        l_seq = int(max(200, rng.normal(read_len, read_len / 3)))
        name = b"%08x-4c1d-4f7a-9c3e-%012d" % (n_reads * 2654435761 & 0xFFFFFFFF, n_reads)
        bases = BASES[rng.integers(0, 4, l_seq)].tobytes()
        qual = rng.integers(0, 51, l_seq).astype(np.uint8)          # a mean error of 0.095: above Q10; halved, 0.18: below it
        if low.random() < 0.3:
            qual >>= 1
        rec = b"@" + name + b" runid=0123abcd ch=%d\n" % (n_reads % 512) + bases + b"\n+\n" + (qual + 33).tobytes() + b"\n"
        parts.append(rec)
        n_bytes += len(rec)
        n_reads += 1
    raw = b"".join(parts)
    del parts
    with open(paths[0], "wb") as f:
        f.write(raw)
    with ProcessPoolExecutor(16) as ex:
        step = BLOCK * 256
        blob = b"".join(ex.map(_bgzf, [raw[k:k + step] for k in range(0, len(raw), step)])) + EOF_BLOCK
    with open(paths[1], "wb") as f:
        f.write(blob)
    print("%d reads, %.0f MB of FASTQ text, %.0f MB as BGZF" % (n_reads, len(raw) / 1e6, len(blob) / 1e6), flush=True)
    return paths


def wall(argv, env=None, inflate=False):
    """the process's wall time with its stdout sent to a pipe that a thread of this process empties -> (seconds, bytes, CRC-32 of stdout — of
    the inflated stdout for a BGZF stream, inflated after the clock has stopped)"""
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    p = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    pieces = []
    while True:
        piece = p.stdout.read(1 << 24)
        if not piece:
            break
        pieces.append(piece)
    err = p.stderr.read()
    rc = p.wait()
    dt = time.perf_counter() - t0
    if rc != 0:
        raise SystemExit("%s failed (%d): %s" % (argv, rc, err.decode(errors="replace")[-2000:]))
    n, crc = 0, 0
    if inflate:
        import gzip
        text = gzip.decompress(b"".join(pieces))
        n, crc = len(text), zlib.crc32(text)
    else:
        for piece in pieces:
            n += len(piece)
            crc = zlib.crc32(piece, crc)
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--old", default=os.path.join(ROOT, "_old", "cornetto"))
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import cornetto_amd
    new = cornetto_amd.CLI_PATH
    old = a.old if os.path.exists(a.old) else new
    print("the positional seq runs %s" % ("the parent commit's binary" if old == a.old else "THIS build's binary (no parent binary at %s): the same host code" % a.old), flush=True)
    plain, gz = synthesize(a.dir, a.mb, a.read, 21)
    m = str(a.min_len)
    if a.kernels:
        acc = cornetto_amd.Accel(0)
        with open(gz, "rb") as f:
            blob = f.read()
        for max_err in (None, 10 ** 8):
            for rep in range(2):
                text, st, _, rest, ok = acc.fastq_seq(blob, a.min_len, window=256 << 20, slab=32 << 20, bgzf_in=True, max_err=max_err)
            tm = {}
            for name, ms in acc.fq_timing:
                tm.setdefault(name, []).append(ms)
            print("kernels of one pass over the .gz file%s (window 256 MiB, slabs of 32 MiB, %d bytes of text, plain %s): %s" % (
                "" if max_err is None else " with -q 10", len(text), ok,
                "; ".join("%s %d x, %.2f ms in all, %.2f ms the longest" % (k, len(v), sum(v), max(v)) for k, v in tm.items())), flush=True)
            ms, nb = acc.fq_text_time
            print("fqseq_text: %d bytes written in %.3f ms: %.0f GB/s of bytes read plus bytes written" % (nb, ms, 2 * nb / ms / 1e6 if ms > 0 else 0), flush=True)
            if max_err is not None:
                ms = sum(tm.get("qmean_sum", [0.0]))
                print("qmean_sum: %d x, %.3f ms over windows of %d bytes in all: %.0f GB/s of window, %.0f GB/s of the %d quality bytes it sums; %d of %d reads >= %d printed" % (
                    len(tm.get("qmean_sum", [])), ms, os.path.getsize(plain), os.path.getsize(plain) / ms / 1e6 if ms > 0 else 0, st[3] / ms / 1e6 if ms > 0 else 0, st[3],
                    acc.fq_qstats[0], st[2], a.min_len), flush=True)
        acc.close()
        return
    cmds = {"parent seq, plain file": ([old, "seq", "-m", m, plain], False), "parent seq, .gz file": ([old, "seq", "-m", m, gz], False),
            "--fastq plain -> plain": ([new, "seq", "-m", m, "--fastq", plain], False), "--fastq gz -> plain": ([new, "seq", "-m", m, "--fastq", gz], False),
            "--fastq gz -> --bgzf": ([new, "seq", "-m", m, "--fastq", gz, "--bgzf"], True),
            "--accel=no --fastq gz --bgzf": ([new, "seq", "-m", m, "--accel=no", "--fastq", gz, "--bgzf"], True)}
    for argv, z in cmds.values():          # (one run of each unmeasured: the files are in the page cache afterwards)
        wall(argv)
    times, outs = {k: [] for k in cmds}, {}
    for _ in range(a.runs):
        for k, (argv, z) in cmds.items():
            dt, n, crc = wall(argv, inflate=z)
            times[k].append(dt)
            outs[k] = (n, crc)
    same = len(set(outs.values())) == 1
    print("-m %s: text %s (%d bytes)" % (m, "the same from all six" if same else "DIFFERS %r" % (outs,), next(iter(outs.values()))[0]), flush=True)
    for k in cmds:
        print("  %-30s %s" % (k, stats(times[k])), flush=True)
    # -q 10 beside the same command without it, alternating
    pairs = {"--fastq plain -> plain": [new, "seq", "-m", m, "--fastq", plain], "--fastq gz -> plain": [new, "seq", "-m", m, "--fastq", gz],
             "positional seq, plain file (this build)": [new, "seq", "-m", m, plain]}
    tq, outq = {(k, q): [] for k in pairs for q in (0, 1)}, {}
    for i in range(a.runs + 1):          # (the first round unmeasured)
        for k, argv in pairs.items():
            for q in (0, 1):
                dt, n, crc = wall(argv + (["-q", "10"] if q else []))
                if i:
                    tq[(k, q)].append(dt)
                outq[(k, q)] = (n, crc)
    same = len(set(outq[(k, 1)] for k in pairs)) == 1
    print("-m %s -q 10: text %s (%d of %d bytes)" % (m, "the same from all three" if same else "DIFFERS %r" % (outq,), outq[(next(iter(pairs)), 1)][0], outq[(next(iter(pairs)), 0)][0]), flush=True)
    for k in pairs:
        print("  %-40s %s   with -q 10: %s" % (k, stats(tq[(k, 0)]), stats(tq[(k, 1)])), flush=True)


if __name__ == "__main__":
    main()
