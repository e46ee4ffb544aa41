#!/usr/bin/env python3
"""One line per kernel of the library: registers, scratch, occupancy and LDS as the compiler reports them
(-Rpass-analysis=kernel-resource-usage, device code only, the flags of cornetto_amd/Makefile).  No GPU needed.

    python tools/resource_usage.py [tree] > profiles/<name>_resource_usage.txt

Two listings (before / after a change) are compared with diff: a kernel whose code did not change has the same line.
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -Wno-inline-asm -ffp-contract=off".split()
FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def one(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                         capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return rows


def main():
    tree = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    os.chdir(os.path.join(tree, "cornetto_amd"))
    srcs = sorted(glob.glob("csrc/*.hip"))
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        per_file = list(ex.map(one, srcs))
    names = [r["name"] for rows in per_file for r in rows]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if names else []
    plain = [re.sub(r"\(anonymous namespace\)::", "", p) for p in plain]
    plain = [re.sub(r"\(.*\)$", "", p) for p in plain]          # the argument list: the template arguments tell instantiations apart
    print("%-14s %5s %5s %5s %7s %4s %6s  %s" % (("file",) + tuple(f[1] for f in FIELDS) + ("kernel",)))
    i = 0
    for src, rows in zip(srcs, per_file):
        for r in rows:
            print("%-14s %5s %5s %5s %7s %4s %6s  %s" % ((os.path.basename(src),) + tuple(r.get(f[0], "?") for f in FIELDS) + (plain[i],)))
            i += 1


if __name__ == "__main__":
    main()
