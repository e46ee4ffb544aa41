#!/usr/bin/env python3
"""development aid: counting read k-mers (kq_count, csrc/kcount.hip) on a seeded 30x sample of the bench's synthetic assembly, as 150-base reads
and as 15 kb reads with substitutions at 1e-3, against the yardstick: kq_insert (the plain set of `cornetto qv`) on the same bases.  Per read
length: time per G k-mers of both kernels, the share of lane-steps that own a base (kq_count deals runs of 16 bases over the batch; kq_insert
gives a record's 4096-base tile a workgroup), then kq_hist and kq_seal on the filled table, all from cornetto_accel_last_timing().  Without
--kernels only the CLI: the wall time of `cornetto qv -r` on the device and with --accel=no on a sample small enough for the host's single thread
(--host-mbases of assembly, 30x of 150-base reads in a FASTQ file).  Not read by bench.py.
   python tools/perf_kcount.py --dir /dev/shm/kcount --kernels"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from perf_kqv import write_fasta  # noqa: E402

RUN, TILE = 16, 4096


def make_reads(torch, bases, offs, lens, L, cover, rate, seed):
    """-> (device tensor [n, stride] of reads of L bases at seeded starts inside the contigs, substitutions at `rate`; stride a multiple of 64)"""
    dev = bases.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    total = int(sum(lens))
    n = int(total * cover / L)
    o = torch.tensor(offs, dtype=torch.int64, device=dev)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    start = torch.randint(0, bases.numel() - L, (n + n // 4,), generator=g, device=dev)
    c = torch.searchsorted(o, start, right=True) - 1
    start = start[(start + L) <= (o[c] + ln[c])][:n]
    stride = (L + 63) // 64 * 64
    reads = torch.full((start.numel(), stride), ord("N"), dtype=torch.uint8, device=dev)
    step = max(1, (1 << 28) // stride)
    for i in range(0, start.numel(), step):
        reads[i:i + step, :L] = bases[start[i:i + step, None] + torch.arange(L, device=dev)[None, :]]
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGTacgt", b"CGTAcgta"):
        lut[a] = b
    flat = reads.view(-1)
    at = torch.randint(0, start.numel(), (int(start.numel() * L * rate),), generator=g, device=dev) * stride + torch.randint(0, L, (int(start.numel() * L * rate),), generator=g, device=dev)
    old = flat[at]
    new = lut[old.long()]
    flat[at] = torch.where(new != 0, new, old)
    return reads


def write_fastq(path, reads, L):
    r = reads[:, :L].cpu().numpy()
    n = r.shape[0]
    m = np.empty((n, 3 + L + 3 + L + 1), dtype=np.uint8)
    m[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    m[:, 3:3 + L] = r
    m[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    m[:, 6 + L:6 + 2 * L] = ord("I")
    m[:, -1] = 10
    with open(path, "wb") as fh:
        fh.write(m.tobytes())


def timed(argv):
    t0 = time.perf_counter()
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, (argv, p.stderr.decode()[-2000:])
    return dt, p.stdout.decode().strip().split("\n")[-1], [ln for ln in p.stderr.decode().split("\n") if ln.startswith("[qv]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=10, help="the assembly the reads of --kernels are sampled from")
    ap.add_argument("--host-mbases", type=float, default=1)
    ap.add_argument("--cover", type=float, default=30)
    ap.add_argument("--rate", type=float, default=1e-3)
    ap.add_argument("--batch-mbases", type=float, default=64, help="bases per count call, as a streamer hands them over")
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--dir", default="/dev/shm/perf_kcount")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import torch
    import cornetto_amd
    from cornetto_amd import synth
    dev = torch.device("cuda", 0)
    os.makedirs(a.dir, exist_ok=True)

    if a.kernels:
        lens = [int(x) for x in synth.contig_lengths(int(a.mbases * 1e6))]
        bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
        offs = [int(o) for o in offs]
        acc = cornetto_amd.Accel(0)
        for L in (150, 15000):
            reads = make_reads(torch, bases, offs, lens, L, a.cover, a.rate, 11)
            n, stride = reads.shape
            per = max(1, int(a.batch_mbases * 1e6) // L)
            slots = int(1.5 * (2 * sum(lens) + n * L * a.rate * a.k)) + 1
            for kernel in ("kq_count", "kq_insert"):
                s = acc.kset(a.k, slots, channels=1 if kernel == "kq_count" else 0)
                ms, steps = 0.0, 0
                for i in range(0, n, per):
                    m = min(per, n - i)
                    asm = acc.asm_wrap(reads[i:i + m].data_ptr(), np.arange(m, dtype=np.int64) * stride, np.full(m, L, dtype=np.int64))
                    (s.count if kernel == "kq_count" else s.add)(asm)
                    ms += dict(acc.last_timing())[kernel]
                    asm.close()
                    runs = m * ((L + RUN - 1) // RUN)
                    steps += (runs + 255) // 256 * 256 * RUN if kernel == "kq_count" else m * ((L + TILE - 1) // TILE) * TILE
                st = s.stats
                print("%5d-base reads  %-9s %9.2f ms  %7.2f ms per G k-mers  %5.1f %% of lane-steps own a base   %d reads, %d k-mers, %d distinct, %d slots (load %.2f)" % (
                    L, kernel, ms, ms / (st[0] / 1e9), 100.0 * n * L / steps, n, st[0], st[1], st[2], st[1] / st[2]), flush=True)
                if kernel == "kq_count":
                    h = s.hist()
                    t_hist = dict(acc.last_timing())["kq_hist"]
                    solid = s.seal(2)
                    t_seal = dict(acc.last_timing())["kq_seal"]
                    print("%5d-base reads  kq_hist   %9.3f ms  kq_seal %9.3f ms  (%d slots)   hist[1] %d  hist[2..] %d  solid at 2: %d" % (
                        L, t_hist, t_seal, slots, int(h[1]), int(h[2:].sum()), solid[0]), flush=True)
                s.close()
            del reads
            torch.cuda.empty_cache()
        acc.close()
        del bases
        torch.cuda.empty_cache()

    if a.host_mbases:
        lens = [int(x) for x in synth.contig_lengths(int(a.host_mbases * 1e6))]
        bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
        offs = [int(o) for o in offs]
        reads = make_reads(torch, bases, offs, lens, 150, a.cover, a.rate, 13)
        rf, af = os.path.join(a.dir, "reads.fq"), os.path.join(a.dir, "asm.fa")
        write_fastq(rf, reads, 150)
        write_fasta(af, lens, offs, bases.cpu().numpy(), 80)
        del bases, reads
        torch.cuda.empty_cache()
        for mode in ("device", "device", "host"):
            dt, row, line = timed([cornetto_amd.CLI_PATH, "qv", "-k", str(a.k)] + (["--accel=no"] if mode == "host" else []) + ["-r", rf, af])
            print("%g Mbp x %g  cli %-6s %7.2f s   %s   %s" % (a.host_mbases, a.cover, mode, dt, row.split("\t", 1)[1], line[0] if line else ""), flush=True)
        os.remove(rf)
        os.remove(af)


if __name__ == "__main__":
    main()
