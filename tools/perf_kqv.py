#!/usr/bin/env python3
"""development aid: `cornetto qv` on the bench's synthetic assembly (3.16 Gbp, 80-column lines, profile uniform) as the truth and a copy with
seeded substitutions at 1e-4 as the query: the wall time of the CLI on the device and with --accel=no, and with --kernels kq_insert and
kq_query through the binding in k-mers per second and bytes of table touched per second (a probe touches one 64-byte line of the table when it
ends in its home line: a lower bound), from cornetto_accel_last_timing().  --host-mbases: the host path on a smaller pair (its single thread
takes minutes per Gbp); 0 leaves it out.  Not read by bench.py.
   python tools/perf_kqv.py --dir /dev/shm/kqv --kernels --host-mbases 100"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pair(mbases, rate, seed):
    """-> (lens, truth bases, query bases) as host uint8 arrays in the resident layout, and the contig offsets"""
    import torch
    from cornetto_amd import synth
    dev = torch.device("cuda", 0)
    lens = synth.contig_lengths(int(mbases * 1e6))
    bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
    truth = bases.cpu().numpy()
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n = bases.numel()
    at = torch.randint(0, n, (int(n * rate),), generator=g, device=dev)
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGTacgt", b"CGTAcgta"):
        lut[a] = b
    old = bases[at].long()
    bases[at] = torch.where(lut[old] != 0, lut[old], bases[at])
    query = bases.cpu().numpy()
    del bases
    torch.cuda.empty_cache()
    return [int(x) for x in lens], [int(o) for o in offs], truth, query


def write_fasta(path, lens, offs, hb, width):
    with open(path + ".tmp", "wb") as fh:
        for i, (o, L) in enumerate(zip(offs, lens)):
            s = hb[o:o + L]
            fh.write(b">ptg%06dl\n" % i)
            k = len(s) // width * width
            m = np.empty((k // width, width + 1), dtype=np.uint8)
            m[:, :width] = s[:k].reshape(-1, width)
            m[:, width] = 10
            fh.write(m.tobytes())
            fh.write(s[k:].tobytes() + (b"\n" if len(s) > k else b""))
    os.replace(path + ".tmp", path)


def timed(argv):
    t0 = time.perf_counter()
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, (argv, p.stderr.decode()[-2000:])
    return dt, p.stdout.decode().strip().split("\n")[-1], [ln for ln in p.stderr.decode().split("\n") if ln.startswith("[qv]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--host-mbases", type=float, default=0)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--rate", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--dir", default="/dev/shm/perf_kqv")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import cornetto_amd
    os.makedirs(a.dir, exist_ok=True)
    for mb, modes in ((a.mbases, ("device",)), (a.host_mbases, ("device", "host"))):
        if not mb:
            continue
        lens, offs, truth, query = make_pair(mb, a.rate, 7)
        tf, qf = os.path.join(a.dir, "truth_%g.fa" % mb), os.path.join(a.dir, "query_%g.fa" % mb)
        write_fasta(tf, lens, offs, truth, a.width)
        write_fasta(qf, lens, offs, query, a.width)
        for mode in modes:
            for rep in range(a.reps if mode == "device" else 1):
                dt, row, line = timed([cornetto_amd.CLI_PATH, "qv", "-k", str(a.k)] + (["--accel=no"] if mode == "host" else []) + [tf, qf])
                print("%g Mbp  cli %-6s run %d  %7.2f s   %s   %s" % (mb, mode, rep, dt, row.split("\t", 1)[1], line[0] if line else ""), flush=True)
        if a.kernels and mb == a.mbases:
            acc = cornetto_amd.Accel(0)
            total = sum(lens)
            ta = acc.asm_upload([truth[o:o + L] for o, L in zip(offs, lens)])
            s = acc.kset(a.k, 2 * total)
            s.add(ta)
            ins = dict(acc.last_timing())["kq_insert"]
            ta.close()
            qa = acc.asm_upload([query[o:o + L] for o, L in zip(offs, lens)])
            for runs in (False, True):
                r = s.query(qa, runs=runs)
                t = dict(acc.last_timing())
                print("kernels  kq_query%s %8.2f ms  %6.2f G k-mers/s  %6.1f GB/s of table lines   missing %d%s" % (
                    " +runs" if runs else "      ", t["kq_query"], int(r[0].sum()) / t["kq_query"] / 1e6, int(r[0].sum()) * 64 / t["kq_query"] / 1e6, int(r[1].sum()),
                    "  rows %d  (%s)" % (len(r[2]), ", ".join("%s %.2f" % (n, ms) for n, ms in acc.last_timing() if n != "kq_query")) if runs else ""), flush=True)
            st = s.stats
            print("kernels  kq_insert      %8.2f ms  %6.2f G k-mers/s  %6.1f GB/s of table lines   %d positions, %d distinct, %d slots (load %.2f)" % (
                ins, st[0] / ins / 1e6, st[0] * 64 / ins / 1e6, st[0], st[1], st[2], st[1] / st[2]), flush=True)
            s.close()
            qa.close()
            acc.close()
        os.remove(tf)
        os.remove(qf)


if __name__ == "__main__":
    main()
