#!/usr/bin/env python3
"""development aid: `cornetto telostats --breaks` on the bench's synthetic assembly (3.16 Gbp, 80-column lines) against the four-command chain
it replaces (test/realtest.sh:65-69 of the reference),

    cornetto fa2bed asm.fa | awk '{print $1"\\t"$3}' > lens;  cornetto sdust asm.fa > sdust;  cornetto telofind asm.fa > telomere;
    cornetto telobreaks lens sdust telomere > breaks

in alternating runs on one box; the two break files must be equal.  --old-cli names another build of the CLI for the chain (the parent
commit's); by default it is this build's, whose four sub-commands are the parent's.  Also plain `cornetto telostats`: what the option adds
to the sub-command it rides on.  --kernels: the device times of the new stage (bk_*, cornetto_telo_breaks) beside those of the bitset
kernels (tb_*, cornetto_telobreaks on the downloaded lists) from the library's own event pairs, on the same assembly in HBM;
--oracle-contigs N adds the CPU oracle's bitsets on the first N contigs.
   python tools/perf_telobreaks.py --dir /dev/shm/tbk --reps 3 --kernels"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perf_telostats import timed, write_fasta   # noqa: E402


def chain(cli, fa, d, env):
    """the four commands, their three text files in d -> (seconds, seconds per command)"""
    lens, sd, tel, out = (os.path.join(d, n) for n in ("c.lens", "c.sdust", "c.telomere", "c.breaks"))
    t = [timed([cli, "fa2bed", fa], lens + ".bed", d, env)]
    t0 = time.perf_counter()
    with open(lens, "wb") as fo:                   # awk '{print $1"\t"$3}'
        for ln in open(lens + ".bed", "rb"):
            f = ln.split()
            fo.write(f[0] + b"\t" + f[2] + b"\n")
    t[0] += time.perf_counter() - t0
    t.append(timed([cli, "sdust", fa], sd, d, env))
    t.append(timed([cli, "telofind", fa], tel, d, env))
    t.append(timed([cli, "telobreaks", lens, sd, tel], out, d, env))
    return sum(t), t


def kernel_times(a, profile):
    """the event times of one cornetto_telo_breaks() call and of cornetto_telobreaks() on the same lists, the assembly resident"""
    import torch
    import cornetto_amd
    from cornetto_amd import synth
    lens = synth.contig_lengths(int(a.mbases * 1e6))
    bases, offs = synth.make_assembly(torch, torch.device("cuda", 0), lens, 0xC0FFEE, profile)
    torch.cuda.synchronize()
    acc = cornetto_amd.Accel(0)
    asm = acc.asm_wrap(bases.data_ptr(), np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64))
    for rep in range(3):                           # (the first call allocates the workspaces)
        t0 = time.perf_counter()
        rows = acc.telo_breaks(asm)
        wall = time.perf_counter() - t0
        new = acc.last_timing()
    sd = acc.sdust(asm)
    hits = acc.telofind(asm)
    tel = np.zeros(len(hits), dtype=cornetto_amd.TELROW_DT)
    for k, src in (("ctg", "ctg"), ("start", "start"), ("end", "end")):
        tel[k] = hits[src]
    tel["matched"] = hits["end"] - hits["start"]
    for rep in range(3):
        t0 = time.perf_counter()
        old_rows = acc.telobreaks(np.asarray(lens, dtype=np.int32), sd, tel)
        old_wall = time.perf_counter() - t0
        old = acc.last_timing()
    assert np.array_equal(rows, old_rows), (len(rows), len(old_rows))
    print("%-10s %d intervals, %d telofind rows, %d breaks" % (profile, len(sd), len(hits), len(rows)))
    print("%-10s cornetto_telo_breaks  %.3f ms wall;  %s" % (profile, wall * 1e3, "  ".join("%s %.3f" % (n, ms) for n, ms in new)))
    print("%-10s   of which bk_*       %.3f ms" % (profile, sum(ms for n, ms in new if n.startswith("bk_"))))
    print("%-10s cornetto_telobreaks   %.3f ms wall (lists uploaded);  %s" % (profile, old_wall * 1e3, "  ".join("%s %.3f" % (n, ms) for n, ms in old)), flush=True)
    if a.oracle_contigs > 0:                       # the reference's bitsets on one CPU core, the leading contigs
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_bind as ob
        nc = min(a.oracle_contigs, len(lens))
        m = sd["ctg"] < nc
        sd_o = np.zeros(int(m.sum()), ob.SPAN_DT)
        sd_o["ctg"], sd_o["start"], sd_o["end"] = sd["ctg"][m], sd["start"][m], sd["finish"][m]
        t0 = time.perf_counter()
        exp = ob.telobreaks(np.asarray(lens[:nc], dtype=np.int32), sd_o, tel[tel["ctg"] < nc].astype(ob.TELROW_DT))
        cpu = time.perf_counter() - t0
        got = rows[rows["ctg"] < nc]
        same = exp is not None and len(got) == len(exp) and np.array_equal(got["start"], exp["start"]) and np.array_equal(got["finish"], exp["end"])
        print("%-10s CPU oracle on the first %d contigs (%.0f Mbases): %.3f s, %s" % (profile, nc, sum(int(x) for x in lens[:nc]) / 1e6, cpu,
                                                                                      "equal" if same else "DIFFERENT"), flush=True)
    asm.close()
    acc.close()
    del bases
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=3160)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/perf_telobreaks")
    ap.add_argument("--profiles", default="uniform")
    ap.add_argument("--old-cli", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--oracle-contigs", type=int, default=0, help="with --kernels: time the CPU oracle's bitsets on the first N contigs")
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
        bed, brk = os.path.join(a.dir, "t.bed"), os.path.join(a.dir, "t.breaks")
        parts = []

        def run_chain():
            total, per_command = chain(old, fa, a.dir, env)
            parts.append(per_command)
            return total
        ways = [("telostats --breaks", lambda: timed([new, "telostats", "-b", bed, "--breaks", brk, fa], os.devnull, a.dir, env)),
                ("fa2bed+sdust+telofind+telobreaks", run_chain),
                ("telostats", lambda: timed([new, "telostats", "-b", bed, fa], os.devnull, a.dir, env))]
        times = {}
        for rep in range(a.reps + 1):            # (the first round warms the page cache and the code objects: not counted)
            for name, fn in ways:
                dt = fn()
                if rep:
                    times.setdefault(name, []).append(dt)
            print("  round %d: %s" % (rep, "  ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), flush=True)
        for name, v in times.items():
            print("%-10s %-34s min %.3f  median %.3f  max %.3f s" % (profile, name, min(v), sorted(v)[len(v) // 2], max(v)))
        print("%-10s the chain's last round: fa2bed+awk %.3f  sdust %.3f  telofind %.3f  telobreaks %.3f s" % ((profile,) + tuple(parts[-1])))
        same = open(brk, "rb").read() == open(os.path.join(a.dir, "c.breaks"), "rb").read()
        print("%-10s lines of the breaks file: %d (%s the chain's), of the sdust BED: %d, of the telofind TSV: %d" %
              (profile, sum(1 for _ in open(brk)), "equal to" if same else "DIFFERENT FROM", sum(1 for _ in open(os.path.join(a.dir, "c.sdust"))),
               sum(1 for _ in open(os.path.join(a.dir, "c.telomere")))), flush=True)
        assert same
        for f in [fa, bed, brk] + [os.path.join(a.dir, n) for n in ("c.lens", "c.lens.bed", "c.sdust", "c.telomere", "c.breaks")]:
            os.remove(f)
        if a.kernels:
            kernel_times(a, profile)


if __name__ == "__main__":
    main()
