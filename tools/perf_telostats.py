#!/usr/bin/env python3
"""development aid: `cornetto telostats` on the bench's synthetic assembly (3.16 Gbp, 80-column lines; profiles uniform and satellite) against
the two sub-commands it replaces the front of — `cornetto telofind asm.fa > tsv`, then `cornetto telowin tsv 99.9 0.4 > windows` (what
scripts/telostats.sh runs before its awk and bedtools stages, which have no counterpart here) — in alternating runs on one box.  --old-cli
names another build of the CLI for the two old commands (the parent commit's); by default they are this build's, whose telofind and
telowin are the parent's.  Also `cornetto telofind > /dev/null` alone: the expectation for telostats is "no slower than telofind alone plus
the run-to-run spread".  --trace: one more run of each under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the
host), the kernel totals of the new stage (te_*) beside tw_scan's.
   python tools/perf_telostats.py --dir /dev/shm/ts --reps 5 --trace /dev/shm/ts_prof"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_fasta(a, profile):
    import torch
    from cornetto_amd import synth
    fa = os.path.join(a.dir, "asm_%s.fa" % profile)
    lens = synth.contig_lengths(int(a.mbases * 1e6))
    if os.path.exists(fa):
        return fa, sum(int(x) for x in lens)
    bases, offs = synth.make_assembly(torch, torch.device("cuda", 0), lens, 0xC0FFEE, profile)
    hb = bases.cpu().numpy()
    del bases
    torch.cuda.empty_cache()
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
    return fa, sum(int(x) for x in lens)


def timed(argv, stdout, cwd, env):
    t0 = time.perf_counter()
    with open(stdout, "wb") as fo:
        p = subprocess.run(argv, stdout=fo, stderr=subprocess.PIPE, env=env, cwd=cwd)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, (argv, p.stderr.decode()[-2000:])
    return dt


def kernel_stats(d):
    rows = {}
    for f in glob.glob(d + "/**/*_kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"^void ", "", r["Name"].replace("(anonymous namespace)::", "")).split("(")[0]
            c, ns = rows.get(name, (0, 0.0))
            rows[name] = (c + int(r["Calls"]), ns + float(r["TotalDurationNs"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm/perf_telostats")
    ap.add_argument("--profiles", default="uniform,satellite")
    ap.add_argument("--old-cli", default=None)
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 runs")
    a = ap.parse_args()
    import cornetto_amd
    new = cornetto_amd.CLI_PATH
    old = a.old_cli or new
    os.makedirs(a.dir, exist_ok=True)
    env = dict(os.environ)
    env.pop("CORNETTO_ACCEL", None)
    for profile in a.profiles.split(","):
        fa, nb = write_fasta(a, profile)
        print("%s: %.1f Mbases, %d bytes of FASTA" % (profile, nb / 1e6, os.path.getsize(fa)), flush=True)
        tsv, win, bed = os.path.join(a.dir, "t.tsv"), os.path.join(a.dir, "t.win"), os.path.join(a.dir, "t.bed")
        ways = [("telostats", lambda: timed([new, "telostats", "-b", bed, fa], os.devnull, a.dir, env)),
                ("telofind>tsv + telowin", lambda: timed([old, "telofind", fa], tsv, a.dir, env) + timed([old, "telowin", tsv, "99.9", "0.4"], win, a.dir, env)),
                ("telofind>/dev/null", lambda: timed([old, "telofind", fa], os.devnull, a.dir, env))]
        times = {}
        for rep in range(a.reps + 1):            # (the first round warms the page cache and the code objects: not counted)
            for name, fn in ways:
                dt = fn()
                if rep:
                    times.setdefault(name, []).append(dt)
            print("  round %d: %s" % (rep, "  ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
        for name, v in times.items():
            print("%-10s %-24s min %.3f  median %.3f  max %.3f s" % (profile, name, min(v), sorted(v)[len(v) // 2], max(v)))
        print("%-10s rows in the BED: %d, lines of the TSV: %d, windows: %d" % (profile, sum(1 for _ in open(bed)), sum(1 for _ in open(tsv)), sum(1 for _ in open(win))),
              flush=True)
        if a.trace:
            for tag, argv, out in (("telostats", [new, "telostats", "-b", bed, fa], os.devnull), ("telofind", [old, "telofind", fa], tsv),
                                   ("telowin", [old, "telowin", tsv, "99.9", "0.4"], win)):
                d = os.path.join(os.path.abspath(a.trace), "%s_%s" % (profile, tag))
                with open(out, "wb") as fo:
                    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + argv, stdout=fo,
                                       stderr=subprocess.PIPE, env=env, cwd=a.dir)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
                ks = kernel_stats(d)
                if not ks:      # (the CLI leaves through _exit() right after its last line, main.c: the profiler may never write its tables)
                    print("%-10s traced %-10s no kernel statistics were written" % (profile, tag), flush=True)
                    continue
                print("%-10s traced %-10s %s" % (profile, tag, "  ".join("%s x%d %.3f ms" % (k, c, ns / 1e6) for k, (c, ns) in sorted(ks.items(), key=lambda kv: -kv[1][1])[:12])),
                      flush=True)
        for f in (fa, tsv, win, bed):
            os.remove(f)


if __name__ == "__main__":
    main()
