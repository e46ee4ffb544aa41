#!/usr/bin/env python3
"""development aid: `cornetto trioeval` on the bench's synthetic assembly (3.16 Gbp, 80-column lines, profile uniform) split into two "parents" —
the assembly with seeded substitutions at --rate each, at different offsets — and a mosaic query that takes stretches of --stretch bases from
either parent in turn: the wall time of the CLI on the device, and with --kernels kt_insert, kt_mark, kt_tile and kt_seam through the binding,
from cornetto_accel_last_timing().  The yardstick for kt_insert and kt_mark is kq_insert and kq_query on the same input in the same run: the
same two parents into a plain set of the same size, the same query probed against it.  Not read by bench.py.
   python tools/perf_trioeval.py --dir /dev/shm/ktrio --kernels"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perf_kqv import write_fasta  # noqa: E402


def make_trio(mbases, rate, stretch):
    """-> (lens, offs, pat, mat, query) as host uint8 arrays in the resident layout"""
    import torch
    from cornetto_amd import synth
    dev = torch.device("cuda", 0)
    lens = synth.contig_lengths(int(mbases * 1e6))
    bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
    n = bases.numel()
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGTacgt", b"CGTAcgta"):
        lut[a] = b
    parents = []
    for seed in (11, 12):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        p = bases.clone()
        at = torch.randint(0, n, (int(n * rate),), generator=g, device=dev)
        old = p[at].long()
        p[at] = torch.where(lut[old] != 0, lut[old], p[at])
        parents.append(p)
    del bases
    query = parents[0].clone()
    step = 1 << 28
    for lo in range(0, n, step):          # the odd stretches from the other parent, a piece at a time
        hi = min(n, lo + step)
        odd = (torch.arange(lo, hi, device=dev) // stretch) & 1
        query[lo:hi] = torch.where(odd == 1, parents[1][lo:hi], query[lo:hi])
    out = [t.cpu().numpy() for t in parents + [query]]
    del parents, query
    torch.cuda.empty_cache()
    return [int(x) for x in lens], [int(o) for o in offs], out[0], out[1], out[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--rate", type=float, default=5e-4)
    ap.add_argument("--stretch", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--dir", default="/dev/shm/perf_ktrio")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import cornetto_amd
    os.makedirs(a.dir, exist_ok=True)
    lens, offs, pat, mat, query = make_trio(a.mbases, a.rate, a.stretch)
    total = sum(lens)
    if a.kernels:
        acc = cornetto_amd.Accel(0)
        cut = lambda hb: [hb[o:o + L] for o, L in zip(offs, lens)]  # noqa: E731
        t = {}
        for tagged in (False, True):
            s = acc.kset(a.k, 4 * total)
            ins = 0.0
            for tag, hb in ((1, pat), (2, mat)):
                pa = acc.asm_upload(cut(hb))
                s.add(pa, tag=tag if tagged else 0)
                ins += dict(acc.last_timing())["kt_insert" if tagged else "kq_insert"]
                pa.close()
            t["kt_insert" if tagged else "kq_insert"] = ins
            st = s.stats
            qa = acc.asm_upload(cut(query))
            if tagged:
                r = s.phase(qa)
                t.update(dict(acc.last_timing()))
            else:
                km, ms = s.query(qa)
                t["kq_query"] = dict(acc.last_timing())["kq_query"]
            qa.close()
            s.close()
        kmers = int(r[:, 0].sum())
        print("%g Mbp  parents %d positions, %d distinct, %d slots (load %.2f)   query %d k-mers, %d missing (plain set); pat %d mat %d pairs %d switches %d hamming %d" % (
            a.mbases, st[0], st[1], st[2], st[1] / st[2], kmers, int(ms.sum()), int(r[:, 1].sum()), int(r[:, 2].sum()), int(r[:, 3:].sum()),
            int((r[:, 4] + r[:, 5]).sum()), int(r[:, 1:3].min(axis=1).sum())), flush=True)
        for kt, kq, n in (("kt_insert", "kq_insert", st[0]), ("kt_mark", "kq_query", kmers)):
            print("kernels  %-10s %8.2f ms  %6.2f G k-mers/s   %-10s %8.2f ms   ratio %.2f" % (kt, t[kt], n / t[kt] / 1e6, kq, t[kq], t[kt] / t[kq]), flush=True)
        print("kernels  kt_tile    %8.3f ms   kt_seam %8.3f ms   together %.3f ms = %.3f of kt_mark   (%d tiles, %.1f GB/s of bitmap read by kt_tile)" % (
            t["kt_tile"], t["kt_seam"], t["kt_tile"] + t["kt_seam"], (t["kt_tile"] + t["kt_seam"]) / t["kt_mark"], -(-total // 4096),
            total / 4 / t["kt_tile"] / 1e6), flush=True)
        acc.close()
    files = [os.path.join(a.dir, "%s_%g.fa" % (n, a.mbases)) for n in ("pat", "mat", "query")]
    for f, hb in zip(files, (pat, mat, query)):
        write_fasta(f, lens, offs, hb, a.width)
    for rep in range(a.reps):
        t0 = time.perf_counter()
        p = subprocess.run([cornetto_amd.CLI_PATH, "trioeval", "-k", str(a.k)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        line = [ln for ln in p.stderr.decode().split("\n") if ln.startswith("[trioeval]")]
        print("%g Mbp  cli device run %d  %7.2f s   %s   %s" % (a.mbases, rep, dt, p.stdout.decode().strip().split("\n")[-1].split("\t", 1)[1], line[0] if line else ""), flush=True)
    for f in files:
        os.remove(f)


if __name__ == "__main__":
    main()
