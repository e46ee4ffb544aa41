#!/usr/bin/env python3
"""development aid: the copies of an assembly and the copy-number spectrum (kq_copies, kq_spectrum, csrc/kcount.hip) on the table and reads of
tools/perf_kcount.py — a seeded 30x sample of 150-base reads with substitutions at 1e-3 of the bench's synthetic assembly, counted into a table of
1.5 slots per expected key.  With --kernels, from cornetto_accel_last_timing(), alternating in one process:
  kq_copies of the assembly into the counted set (cleared in front of every repeat) against kq_insert of the same assembly into a plain set of the
  same slots — the first of either on its table as it stands (kq_insert: empty, every key new; kq_copies: the reads' keys present), the repeats
  with every key present;
  kq_spectrum against kq_hist on the same table.
Then the CLI: the wall time of `cornetto qv -r reads.fq asm.fa` on the device with and without `--completeness --spectra-cn`, alternating
(--cli-mbases of assembly; 0 skips it).  Not read by bench.py.
   python tools/perf_kspec.py --dir /dev/shm/kspec --kernels"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from perf_kcount import make_reads, timed, write_fastq  # noqa: E402
from perf_kqv import write_fasta  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=10, help="the assembly of --kernels")
    ap.add_argument("--cli-mbases", type=float, default=10)
    ap.add_argument("--cover", type=float, default=30)
    ap.add_argument("--rate", type=float, default=1e-3)
    ap.add_argument("--batch-mbases", type=float, default=64, help="bases per count call, as a streamer hands them over")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--dir", default="/dev/shm/perf_kspec")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import torch
    import cornetto_amd
    from cornetto_amd import synth
    dev = torch.device("cuda", 0)
    os.makedirs(a.dir, exist_ok=True)
    L = 150

    if a.kernels:
        lens = [int(x) for x in synth.contig_lengths(int(a.mbases * 1e6))]
        bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
        offs = [int(o) for o in offs]
        acc = cornetto_amd.Accel(0)
        reads = make_reads(torch, bases, offs, lens, L, a.cover, a.rate, 11)
        n, stride = reads.shape
        per = max(1, int(a.batch_mbases * 1e6) // L)
        slots = int(1.5 * (2 * sum(lens) + n * L * a.rate * a.k)) + 1
        s = acc.kset(a.k, slots, channels=1)
        for i in range(0, n, per):
            m = min(per, n - i)
            r = acc.asm_wrap(reads[i:i + m].data_ptr(), np.arange(m, dtype=np.int64) * stride, np.full(m, L, dtype=np.int64))
            s.count(r)
            r.close()
        st = s.stats
        print("table: %d slots, %d distinct keys of %d read k-mers (load %.2f); assembly %d bases in %d contigs" % (slots, st[1], st[0], st[1] / slots, sum(lens), len(lens)), flush=True)
        asm = acc.asm_wrap(bases.data_ptr(), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64))
        plain = acc.kset(a.k, slots)
        t = {"kq_copies": [], "kq_insert": []}
        for rep in range(a.reps + 1):
            s.copies_clear()
            s.copies(asm)
            t["kq_copies"].append(dict(acc.last_timing())["kq_copies"])
            plain.add(asm)
            t["kq_insert"].append(dict(acc.last_timing())["kq_insert"])
        kmers = plain.stats[0] // (a.reps + 1)
        for name in ("kq_copies", "kq_insert"):
            v = t[name]
            print("%-11s first %8.3f ms   repeats: median %8.3f ms  min %8.3f  max %8.3f  (%d)   %7.2f ms per G k-mers (median)" % (
                name, v[0], statistics.median(v[1:]), min(v[1:]), max(v[1:]), len(v) - 1, statistics.median(v[1:]) / (kmers / 1e9)), flush=True)
        print("kq_copies / kq_insert: first %.2f, repeats (medians) %.2f" % (t["kq_copies"][0] / t["kq_insert"][0], statistics.median(t["kq_copies"][1:]) / statistics.median(t["kq_insert"][1:])),
              flush=True)
        t = {"kq_spectrum": [], "kq_hist": []}
        for rep in range(a.reps + 1):
            spec, solid, found = s.spectrum(2)
            t["kq_spectrum"].append(dict(acc.last_timing())["kq_spectrum"])
            h = s.hist()
            t["kq_hist"].append(dict(acc.last_timing())["kq_hist"])
        assert spec[:, 1:].sum(0).tolist() == h[1:].tolist()
        for name in ("kq_spectrum", "kq_hist"):
            v = t[name][1:]
            print("%-11s median %8.3f ms  min %8.3f  max %8.3f  (%d; %d slots)" % (name, statistics.median(v), min(v), max(v), len(v), slots), flush=True)
        top = sorted(((int(spec[i, c]), i, c) for i in range(spec.shape[0]) for c in range(spec.shape[1]) if spec[i, c]), reverse=True)[:4]
        print("kq_spectrum / kq_hist (medians) %.2f   solid at 2: %d, found %d (%.6f); assembly-only keys %d; the fullest cells (keys, copies, count): %s" % (
            statistics.median(t["kq_spectrum"][1:]) / statistics.median(t["kq_hist"][1:]), solid, found, found / max(solid, 1), int(spec[:, 0].sum()), top), flush=True)
        asm.close()
        plain.close()
        s.close()
        acc.close()
        del reads, bases
        torch.cuda.empty_cache()

    if a.cli_mbases:
        lens = [int(x) for x in synth.contig_lengths(int(a.cli_mbases * 1e6))]
        bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE, "uniform")
        offs = [int(o) for o in offs]
        reads = make_reads(torch, bases, offs, lens, L, a.cover, a.rate, 13)
        rf, af, sf = os.path.join(a.dir, "reads.fq"), os.path.join(a.dir, "asm.fa"), os.path.join(a.dir, "spectra.tsv")
        write_fastq(rf, reads, L)
        write_fasta(af, lens, offs, bases.cpu().numpy(), 80)
        del bases, reads
        torch.cuda.empty_cache()
        for rep in range(3):
            for name, extra in (("plain", []), ("options", ["--completeness", "--spectra-cn", sf])):
                dt, row, line = timed([cornetto_amd.CLI_PATH, "qv", "-k", str(a.k), "-r", rf] + extra + [af])
                print("%g Mbp x %g  cli %-8s %7.2f s   %s   %s" % (a.cli_mbases, a.cover, name, dt, row.split("\t", 1)[1], line[0] if line else ""), flush=True)
        for f in (rf, af, sf):
            os.remove(f)


if __name__ == "__main__":
    main()
