#!/usr/bin/env python3
"""development aid: the evaluation sub-commands `cornetto nx | report | telocontigs` on the bench's synthetic assembly (3.16 Gbp, 80-column
lines), three ways in alternating runs on one box: the device path (names and lengths framed on the GPU), CORNETTO_ACCEL=no (the sequential
reader) and the reference binary (oracle/_ref/cornetto, where it is built); also `report` over four links to the same file.  Every way must
print the same stdout (sha256).
   python tools/perf_eval.py --dir /dev/shm/ev --reps 3"""
import argparse
import hashlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref", "cornetto")


def write_inputs(a, d):
    fa = os.path.join(d, "asm%d.fa" % a.width)
    import bench
    lens = bench.contig_lengths(int(a.mbases * 1e6))
    if not os.path.exists(fa):
        import torch
        bases, offs = bench.make_assembly(torch, torch.device("cuda", 0), lens, 0xC0FFEE)
        hb = bases.cpu().numpy()
        with open(fa + ".tmp", "wb") as fh:
            for i, (o, L) in enumerate(zip(offs, lens)):
                s = hb[int(o):int(o) + int(L)]
                fh.write(b">ptg%06dl\n" % i)
                k = len(s) // a.width * a.width
                m = np.empty((k // a.width, a.width + 1), dtype=np.uint8)
                m[:, :a.width] = s[:k].reshape(-1, a.width)
                m[:, a.width] = 10
                fh.write(m.tobytes())
                fh.write(s[k:].tobytes() + (b"\n" if len(s) > k else b""))
        os.replace(fa + ".tmp", fa)
        del bases
        torch.cuda.empty_cache()
    bed = os.path.join(d, "telo.bed")
    with open(bed, "w") as fh:          # (the bench assembly has 100 contigs: where the reference's telocontigs counts are defined)
        for i in range(0, len(lens), 3):
            fh.write("ptg%06dl\t0\t2000\n" % i)
        fh.write("ptg%06dl\t%d\t%d\n" % (1, lens[1] - 2000, lens[1]))
    links = []
    for k in range(4):                  # four names of one file: `report` over a series of assemblies
        p = os.path.join(d, "copy%d.fa" % k)
        if not os.path.exists(p):
            os.link(fa, p)
        links.append(p)
    return fa, bed, links, sum(int(x) for x in lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/perf_eval")
    a = ap.parse_args()
    import cornetto_amd
    os.makedirs(a.dir, exist_ok=True)
    fa, bed, links, nb = write_inputs(a, a.dir)
    print("assembly: %.1f Mbases, %d bytes of FASTA" % (nb / 1e6, os.path.getsize(fa)), flush=True)
    cmds = [("nx", ["nx", fa]), ("report", ["report", fa]), ("telocontigs", ["telocontigs", fa, bed]), ("report x4", ["report"] + links)]
    env = dict(os.environ)
    env.pop("CORNETTO_ACCEL", None)
    ways = [("device", cornetto_amd.CLI_PATH, env), ("host", cornetto_amd.CLI_PATH, dict(env, CORNETTO_ACCEL="no"))]
    if os.path.exists(REF):
        ways.append(("reference", REF, env))
    times, sums = {}, {}
    for rep in range(a.reps):
        for cname, argv in cmds:
            for wname, b, e in ways:
                t0 = time.perf_counter()
                p = subprocess.run([b] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
                dt = time.perf_counter() - t0
                assert p.returncode == 0, (cname, wname, p.stderr.decode()[-2000:])
                times.setdefault((cname, wname), []).append(dt)
                sums.setdefault(cname, {}).setdefault(wname, set()).add(hashlib.sha256(p.stdout).hexdigest())
        print("rep %d: %s" % (rep, " ".join("%s/%s %.3f s" % (k[0], k[1], v[-1]) for k, v in times.items())), flush=True)
    for (cname, wname), v in times.items():
        print("%-12s %-9s best %.3f s, median %.3f s (%.2f Gbases/s)" % (cname, wname, min(v), sorted(v)[len(v) // 2],
                                                                        nb * (4 if "x4" in cname else 1) / min(v) / 1e9))
    ok = True
    for cname, by in sums.items():
        hs = set().union(*by.values())
        ok &= len(hs) == 1 and all(len(x) == 1 for x in by.values())
        print("sha256 %-12s %s" % (cname, " ".join("%s=%s" % (w, sorted(x)[0][:16]) for w, x in by.items())))
    print("identical:", ok)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
