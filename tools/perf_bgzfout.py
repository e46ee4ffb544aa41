#!/usr/bin/env python3
"""development aid: `seq --bam --bgzf` on the synthetic long-read BAM of tools/perf_bamfq.py (random bases and qualities: 2 and 5.7 bits of
the 8 of a byte), output to a FILE, alternating on one box:
   plain        `seq --bam` to a plain file — the parent commit's binary (`_old/cornetto` beside `_old/libcornetto_hip.so`) when it is there,
                this build's otherwise: the code of that path is the same
   host bgzf    `seq --bam --accel=no --bgzf`: the host reader through the zlib writer of cli/bgzf_out.c
   device bgzf  `seq --bam --bgzf`: the slab deflated on the device, only members cross the bus
   python tools/perf_bgzfout.py --dir /tmp/bamfq [--mb 500] [--runs 5] [--old _old/cornetto] [--kernels] [--deflate-only]
prints: the wall times, the sizes of the three files, that both BGZF files gunzip to the plain one, the size of the device's stream against
zlib level 1 and level 6 over the same 65280-byte pieces (of the first --sample MB of the text); with --kernels the event times of
bgzf_deflate / bgzf_scan / bgzf_pack of one cornetto_text_deflate() call over the first --sample MB of the text, per GB of text; with
--deflate-only nothing but three such calls over the text an earlier run left in --dir: the program for `rocprofv3 --kernel-trace --stats --
python tools/perf_bgzfout.py --dir D --deflate-only`, a run of its own (the CLI leaves through _exit() and a tracer of it writes nothing)."""
import argparse
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import perf_bamfq  # noqa: E402

MEMBER = 65280


def wall_to_file(argv, path):
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        p = subprocess.run(argv, stdout=f, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (argv, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    return dt


def crc_of(path, gz):
    crc, n = 0, 0
    d = zlib.decompressobj(31) if gz else None
    with open(path, "rb") as f:
        while True:
            piece = f.read(1 << 24)
            if not piece:
                break
            if not gz:
                crc, n = zlib.crc32(piece, crc), n + len(piece)
            while gz and piece:
                out = d.decompress(piece)
                crc, n = zlib.crc32(out, crc), n + len(out)
                piece = d.unused_data if d.eof else b""
                if d.eof:                       # the next member
                    d = zlib.decompressobj(31)
    return n, crc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--mb", type=int, default=500)
    ap.add_argument("--read", type=int, default=20000)
    ap.add_argument("--min-len", type=int, default=15000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=128)
    ap.add_argument("--old", default=os.path.join(ROOT, "_old", "cornetto"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--deflate-only", action="store_true")
    a = ap.parse_args()
    import cornetto_amd
    new = cornetto_amd.CLI_PATH
    bam = perf_bamfq.synthesize(a.dir, a.mb, a.read, 0.3, 21)[0]
    m = str(a.min_len)
    if a.deflate_only:
        with open(os.path.join(a.dir, "out.plain"), "rb") as f:
            text = f.read(a.sample << 20)
        acc = cornetto_amd.Accel(0)
        for _ in range(3):
            n = len(acc.bgzf_deflate(text))
        print("cornetto_text_deflate of %d bytes, three times: %d bytes of members" % (len(text), n), flush=True)
        acc.close()
        return
    plain_bin = a.old if os.path.exists(a.old) else new
    print("plain runs %s" % ("the parent commit's binary" if plain_bin == a.old else "this build's seq --bam (no parent binary at %s): the same code" % a.old), flush=True)
    cmds = {"plain": [plain_bin, "seq", "-m", m, "--bam", bam], "host bgzf": [new, "seq", "-m", m, "--accel=no", "--bam", bam, "--bgzf"],
            "device bgzf": [new, "seq", "-m", m, "--bam", bam, "--bgzf"]}
    out = {k: os.path.join(a.dir, "out.%s" % k.replace(" ", "_")) for k in cmds}
    for k in ("plain", "device bgzf"):          # (one run unmeasured: the BAM is in the page cache afterwards)
        wall_to_file(cmds[k], out[k])
    times = {k: [] for k in cmds}
    for r in range(a.runs):
        for k, argv in cmds.items():
            if k == "host bgzf" and r >= max(1, a.runs // 3):      # (one thread of zlib: tens of seconds a run)
                continue
            times[k].append(wall_to_file(argv, out[k]))
    sizes = {k: os.path.getsize(out[k]) for k in cmds}
    want = crc_of(out["plain"], False)
    same = {k: crc_of(out[k], True) == want for k in ("host bgzf", "device bgzf")}
    print("text %d bytes; both BGZF files gunzip to it: %s" % (want[0], same), flush=True)
    for k in cmds:
        print("  %-12s %s   %d bytes (%.3f of the text), %.2f GB/s of text" % (k, perf_bamfq.stats(times[k]), sizes[k], sizes[k] / max(1, want[0]),
                                                                               want[0] / 1e9 / sorted(times[k])[len(times[k]) // 2]), flush=True)
    with open(out["plain"], "rb") as f:
        text = f.read(a.sample << 20)
    n1 = n6 = 0
    for at in range(0, len(text), MEMBER):
        for level in (1, 6):
            z = zlib.compressobj(level, zlib.DEFLATED, -15)
            n = len(z.compress(text[at:at + MEMBER]) + z.flush()) + 26
            n1, n6 = (n1 + n, n6) if level == 1 else (n1, n6 + n)
    acc = cornetto_amd.Accel(0)
    dev = acc.bgzf_deflate(text)
    print("the first %d bytes of the text as members of %d bytes: device %d (%.4f), zlib level 1 %d (%.4f), zlib level 6 %d (%.4f)" % (
        len(text), MEMBER, len(dev), len(dev) / len(text), n1, n1 / len(text), n6, n6 / len(text)), flush=True)
    if a.kernels:
        for _ in range(3):
            acc.bgzf_deflate(text)
            print("cornetto_text_deflate of %d bytes: %s" % (len(text), "; ".join("%s %.3f ms (%.2f ms per GB of text)" % (k, ms, ms / (len(text) / 1e9))
                                                                                  for k, ms in acc.deflate_timing)), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
