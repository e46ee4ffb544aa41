#!/usr/bin/env python3
"""development aid: `cornetto noboringbits` on per-base bedgraphs against `cornetto noboringbits --runs` on the run-length files of the same
coverage, in alternating runs on one box, and the expansion kernel rl_fill against hipMemsetAsync over the same bytes.

The coverage is the bench's configuration 3 (cornetto_amd/synth.py make_coverage) in three profiles: "noise" (the bench's own: noise at every
base, so runs of 1-2 positions — the honest worst case, where --runs saves nothing), "flat" (the noise off: runs of 1 kb) and "readlike" (depth
changes every 300 bases).  Both files are written per base and as maximal runs, from the device, in fixed-width columns (%d reads zero-padded
numbers the same).  The two stdouts must hash equal.

--fill DIR: instead of the CLI comparison, one ingest per profile through the C ABI under `rocprofv3 --kernel-trace --stats` (a child process
of its own, the program after `--`; no counters): the kernel totals of rl_fill beside the fill kernel of the two hipMemsetAsync calls that
cornetto_bgrun_finish() makes over the arrays of the coverage object — the same number of bytes, the same process, the same box.
   python tools/perf_bgruns.py --dir /dev/shm/bgruns --mbases 3160 --reps 3
   python tools/perf_bgruns.py --dir /dev/shm/bgruns --mbases 1000 --fill /dev/shm/bgruns_prof"""
import argparse
import csv
import glob
import hashlib
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = 37      # ptg000000l \t 9 digits \t 9 digits \t 5 digits \n


def rows_text(torch, dev, ctg, start, end, val):
    """rows (contig number, start, end, value) -> bedgraph text, on the device"""
    n = int(ctg.numel())
    out = torch.empty((n, ROW), dtype=torch.uint8, device=dev)
    out[:, :10] = torch.tensor(list(b"ptg000000l"), dtype=torch.uint8, device=dev)
    out[:, 10] = 9
    out[:, 20] = 9
    out[:, 30] = 9
    out[:, 36] = 10

    def digits(v, col, nd):
        v = v.clone()
        for k in range(nd):
            out[:, col + nd - 1 - k] = (v % 10 + 48).to(torch.uint8)
            v //= 10

    digits(ctg, 3, 6)
    digits(start, 11, 9)
    digits(end, 21, 9)
    digits(val, 31, 5)
    return out.reshape(-1)


def write_pair(torch, dev, a, profile, per_base):
    """-> {kind: (path total, path mq)}, positions, {path: records}"""
    from cornetto_amd import synth
    lens = synth.contig_lengths(int(a.mbases * 1e6))
    offs = np.zeros(len(lens), dtype=np.int64)
    for i in range(1, len(lens)):
        offs[i] = offs[i - 1] + (lens[i - 1] + 63) // 64 * 64
    depth, mq = synth.make_coverage(torch, dev, lens, offs, 0xC0FFEE, profile)
    paths, n_rec = {}, {}
    for kind in (("base", "runs") if per_base else ("runs",)):
        paths[kind] = tuple(os.path.join(a.dir, "%s.%s.%s.bg" % (profile, kind, nm)) for nm in ("total", "mq20"))
        for arr, path in zip((depth, mq), paths[kind]):
            n_rec[path] = 0
            with open(path, "wb") as fh:
                for ci, (o, n) in enumerate(zip(offs, lens)):
                    for s in range(0, int(n), a.chunk):      # (a chunk ends a run: the files stay valid, adjacent runs of equal value are allowed)
                        e = min(int(n), s + a.chunk)
                        v = arr[int(o) + s:int(o) + e].to(torch.int64) & 0xFFFF
                        if kind == "base":
                            st = torch.arange(s, e, device=dev, dtype=torch.int64)
                            en = st + 1
                        else:
                            first = torch.ones(e - s, dtype=torch.bool, device=dev)
                            first[1:] = v[1:] != v[:-1]
                            st = torch.nonzero(first).reshape(-1) + s
                            en = torch.cat([st[1:], torch.tensor([e], device=dev, dtype=torch.int64)])
                            v = v[st - s]
                        ctg = torch.full_like(st, ci + 1)
                        fh.write(rows_text(torch, dev, ctg, st, en, v).cpu().numpy().tobytes())
                        n_rec[path] += int(st.numel())
    del depth, mq
    if dev.type == "cuda":
        torch.cuda.empty_cache()
    return paths, int(sum(int(x) for x in lens)), n_rec


def timed(argv, env, cwd):
    t0 = time.perf_counter()
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, (argv, p.stderr.decode()[-2000:])
    return dt, hashlib.sha256(p.stdout).hexdigest(), len(p.stdout)


def kernel_stats(d):
    rows = {}
    for f in glob.glob(d + "/**/*_kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"^void ", "", r["Name"].replace("(anonymous namespace)::", "")).split("(")[0]
            c, ns = rows.get(name, (0, 0.0))
            rows[name] = (c + int(r["Calls"]), ns + float(r["TotalDurationNs"]))
    return rows


def dispatches(d):
    """-> {kernel name: [duration in ns of every dispatch]} from the kernel trace"""
    out = {}
    for f in glob.glob(d + "/**/*_kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"^void ", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).split("(")[0]
            out.setdefault(name, []).append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    return out


def fill_child(a):
    """one ingest of the run files of --fill-child's profile through the C ABI (the process rocprofv3 traces)"""
    import cornetto_amd
    acc = cornetto_amd.Accel(0)
    t, q = (os.path.join(a.dir, "%s.runs.%s.bg" % (a.fill_child, nm)) for nm in ("total", "mq20"))

    def pieces(path):
        with open(path, "rb") as fh:
            while True:
                b = fh.read(a.piece)
                if not b:
                    return
                yield b
    for rep in range(2):          # (the first ingest loads the code objects and grows the work spaces)
        cov, names, ncl = acc.bedgraph_runs_ingest(pieces(t), pieces(q), alternate=False)
        print("fill child %s: %d contigs, %d positions" % (a.fill_child, len(names), sum(cov.lens)), flush=True)
        cov.close()
    acc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/perf_bgruns")
    ap.add_argument("--profiles", default="noise,flat,readlike")
    ap.add_argument("--chunk", type=int, default=1 << 24, help="positions formatted at a time")
    ap.add_argument("--piece", type=int, default=64 << 20, help="--fill: bytes per feed")
    ap.add_argument("--device", default="cuda", help="where the text is generated (cpu: a rehearsal, with --accel no)")
    ap.add_argument("--accel", default="yes")
    ap.add_argument("--fill", default=None, help="directory for the rocprofv3 runs of the expansion alone")
    ap.add_argument("--fill-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--keep", action="store_true")
    a = ap.parse_args()
    if a.fill_child:
        return fill_child(a)
    import torch
    import cornetto_amd
    dev = torch.device(a.device, 0) if a.device == "cuda" else torch.device("cpu")
    cli = cornetto_amd.CLI_PATH
    os.makedirs(a.dir, exist_ok=True)
    env = dict(os.environ)
    env.pop("CORNETTO_ACCEL", None)
    for profile in a.profiles.split(","):
        paths, n_pos, n_rec = write_pair(torch, dev, a, profile, per_base=not a.fill)
        for kind, pp in paths.items():
            print("%-9s %-5s %.1f M positions: %s" % (profile, kind, n_pos / 1e6, "  ".join(
                "%s %d bytes, %d records, mean run %.2f" % (os.path.basename(p), os.path.getsize(p), n_rec[p], n_pos / max(1, n_rec[p])) for p in pp)), flush=True)
        if a.fill:
            d = os.path.join(os.path.abspath(a.fill), profile)
            p = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                                os.path.abspath(__file__), "--dir", a.dir, "--piece", str(a.piece), "--fill-child", profile],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            print(p.stdout.decode().strip(), flush=True)
            ks = kernel_stats(d)
            for k, (c, ns) in sorted(ks.items(), key=lambda kv: -kv[1][1])[:14]:
                print("%-9s traced %-44s x%-6d %10.3f ms" % (profile, k, c, ns / 1e6), flush=True)
            dp = dispatches(d)
            fill = sum(sum(v) for k, v in dp.items() if k.startswith("rl_fill"))
            # the memsets of the same bytes: the two arrays of the coverage object in each of the two ingests — the four longest fill dispatches
            # (the others are the 256-byte clears of the feeds)
            big = sorted((x for k, v in dp.items() if "fillBuffer" in k for x in v), reverse=True)[:4]
            mset = sum(big)
            runs = (n_rec[paths["runs"][0]] + n_rec[paths["runs"][1]]) / 2
            print("%-9s rl_fill %.3f ms in %d dispatches for %d bytes; hipMemsetAsync over the same bytes %.3f ms in 4 dispatches (%s ms each); observed factor "
                  "%.2f, modelled 1 + 12 / (2 x mean run) = %.2f" % (profile, fill / 1e6, sum(len(v) for k, v in dp.items() if k.startswith("rl_fill")), 2 * 2 * 2 * n_pos,
                                                                     mset / 1e6, " ".join("%.3f" % (x / 1e6) for x in big), fill / mset if mset else float("nan"),
                                                                     1 + 12 / (2 * n_pos / runs)), flush=True)
        else:
            opts = ["--accel=" + a.accel]
            ways = [("per base", [cli, "noboringbits"] + opts + [paths["base"][0], "-q", paths["base"][1]]),
                    ("--runs", [cli, "noboringbits", "--runs"] + opts + [paths["runs"][0], "-q", paths["runs"][1]])]
            times, hashes = {}, {}
            for rep in range(a.reps + 1):            # (the first round warms the page cache and the code objects: not counted)
                for name, argv in ways:
                    dt, hx, nb = timed(argv, env, a.dir)
                    hashes[name] = (hx, nb)
                    if rep:
                        times.setdefault(name, []).append(dt)
                print("  round %d: %s" % (rep, "  ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
            assert hashes["per base"] == hashes["--runs"], hashes
            for name, v in times.items():
                print("%-9s %-9s min %.3f  median %.3f  max %.3f s" % (profile, name, min(v), sorted(v)[len(v) // 2], max(v)))
            print("%-9s stdout: %d bytes, sha256 %s (equal)" % (profile, hashes["--runs"][1], hashes["--runs"][0][:16]), flush=True)
        if not a.keep:
            for pp in paths.values():
                for p in pp:
                    os.remove(p)


if __name__ == "__main__":
    main()
