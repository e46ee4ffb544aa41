#!/usr/bin/env python3
"""development aid: what the haplotype stage of the diploid panel (`noboringbits --panel --hap`, cornetto_hap_fun) costs.

A synthetic PAF pair (two haplotypes, --rows rows each, default 10^5 and 10^6) over the 100 contigs of tests/golden/bigenough/chroms.bed, then
  1. the device call: cornetto_hap_fun() through the binding, the kernel times of cornetto_accel_last_timing() summed per stage (device events)
     and the wall time of the call (it ends in a synchronise), after one warm-up call, median of --reps;
  2. the CLI with and without --accel=no on a small coverage pair (the committed fixtures): wall time of the process, alternating, median;
  3. one pass with --dip against two separate runs (primary, diploid): wall time, alternating, median.
The coverage is small on purpose: 2 and 3 measure the haplotype stage and the process around it, not the ingest.  Needs a GPU: no fallback.
   python tools/perf_hap.py --dir /dev/shm/perf_hap --reps 5"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def assembly():
    names, lens = [], []
    for l in open(os.path.join(ROOT, "tests", "golden", "bigenough", "chroms.bed"), "rb"):
        n, a, b = l.split()
        names.append(n)
        lens.append(int(b) - int(a))
    return names, lens


def make_rows(rng, lens, n, n_queries):
    """n alignment rows: chains of a query on a target, in file order of a shuffled PAF -> (query, ctg, start, end) arrays"""
    L = np.asarray(lens, dtype=np.int64)
    ctg = rng.choice(len(lens), size=n, p=L / L.sum())
    query = rng.integers(0, n_queries, size=n)
    start = (rng.random(n) * (L[ctg] - 1)).astype(np.int64)
    end = np.minimum(start + rng.integers(200, 60_000, size=n), L[ctg])
    return query.astype(np.int32), ctg.astype(np.int32), start.astype(np.int32), end.astype(np.int32)


def write_paf(path, names, lens, rows, tag):
    q, c, s, e = rows
    with open(path, "wb") as fh:
        for i in range(len(q)):
            fh.write(b"%s%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t60\ttp:A:P\n" % (tag, q[i], e[i] - s[i], e[i] - s[i], names[c[i]], lens[c[i]], s[i], e[i], e[i] - s[i],
                                                                                    e[i] - s[i]))


def timed(args):
    t0 = time.perf_counter()
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(args), p.stderr.decode()[-2000:]))
    return dt, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_hap.py measures on the GPU: none found")
    import cornetto_amd
    os.makedirs(a.dir, exist_ok=True)
    names, lens = assembly()
    g = os.path.join(ROOT, "tests", "golden")
    cov = []
    for f in ("cov-total.bg", "cov-mq20.bg"):
        cov.append(os.path.join(a.dir, f))
        open(cov[-1], "wb").write(gzip.open(os.path.join(g, f + ".gz")).read())
    asm_bed = os.path.join(g, "bigenough", "chroms.bed")
    acc = cornetto_amd.Accel(0)
    for n in a.rows:
        rng = np.random.default_rng(n)
        haps = [make_rows(rng, lens, n, max(1, n // 200)) for _ in range(2)]
        dev_rows = []
        pafs = []
        for k, r in enumerate(haps):
            d = np.zeros(n, cornetto_amd.HAP_ROW_DT)
            d["query"], d["ctg"], d["start"], d["finish"] = r
            dev_rows.append(d)
            pafs.append(os.path.join(a.dir, "hap%d.%d.paf" % (k + 1, n)))
            write_paf(pafs[-1], names, lens, r, b"h%dq" % (k + 1))
        # 1. the device call
        fun = acc.hap_fun(lens, dev_rows)                                     # warm-up: code objects, workspaces
        wall, kern, stages = [], [], {}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            acc.hap_fun(lens, dev_rows)
            wall.append(time.perf_counter() - t0)
            C = cornetto_amd.C
            m = acc.L.cornetto_accel_last_timing(acc.h, None, None, 0)
            nm, ms = (C.c_char_p * m)(), (C.c_float * m)()
            acc.L.cornetto_accel_last_timing(acc.h, nm, ms, m)
            kern.append(sum(ms))
            st = {}
            for x, y in zip(nm, ms):
                st[x.decode()] = st.get(x.decode(), 0.0) + y
            for k, v in st.items():
                stages.setdefault(k, []).append(v)
        res = {"rows_per_hap": n, "funbits": int(len(fun)), "device_call_wall_ms": round(statistics.median(wall) * 1e3, 3),
               "device_kernels_ms": round(statistics.median(kern), 3), "launches": m,
               "stages_ms": {k: round(statistics.median(v), 3) for k, v in sorted(stages.items())}}
        # 2. and 3. the CLI
        base = [cornetto_amd.CLI_PATH, "noboringbits", cov[0], "-q", cov[1], "--panel", asm_bed]
        hap = ["--hap", pafs[0], "--hap", pafs[1]]
        dip = os.path.join(a.dir, "dip.%d.bed" % n)
        t = {"cli_dev": [], "cli_host": [], "one_pass_dip": [], "two_runs": []}
        outs = {}
        for _ in range(a.reps + 1):                                           # (the first round is the warm-up: page cache, code objects)
            d1, o1 = timed(base + hap)
            d2, o2 = timed(base[:2] + ["--accel=no"] + base[2:] + hap)
            d3, o3 = timed(base + hap + ["--dip", dip])
            d4, o4 = timed(base)
            if o1 != o2 or open(dip, "rb").read() != o1 or o3 != o4:
                sys.exit("the device path, the host path and the one-pass run disagree at %d rows" % n)
            outs = {"diploid_rows": o1.count(b"\n"), "primary_rows": o4.count(b"\n")}
            t["cli_dev"].append(d1); t["cli_host"].append(d2); t["one_pass_dip"].append(d3); t["two_runs"].append(d1 + d4)
        res.update(outs)
        res.update({k + "_s": round(statistics.median(v[1:]), 4) for k, v in t.items()})
        print(json.dumps(res), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
