#!/bin/bash
# development aid: `cornetto sdust` / `telofind` on the bench assembly (FASTA in /dev/shm) with two builds of the CLI, alternating on one box:
#   bash tools/cli_ab.sh <cornetto A> <cornetto B> [runs per binary and sub-command, default 10]
# One unused warm-up run per binary and sub-command, then the runs; median and range per binary, one stdout hash per binary (must be equal).
# PIECES=1 adds one run of B with CORNETTO_CLI_WHOLE=0 (the piece loop: a test mode, for the record).
A=${1:?two cornetto binaries}; B=${2:?two cornetto binaries}; N=${3:-10}
python3 - <<'PY' || exit 1
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from cornetto_amd import synth
dev = torch.device("cuda", 0)
lens = synth.contig_lengths(0)
bases, offs = synth.make_assembly(torch, dev, lens, 0xC0FFEE)
hb = bases.cpu().numpy()
with open("/dev/shm/asm1.fa", "wb") as f:
    for i, (o, L) in enumerate(zip(offs, lens)):
        f.write(b">ptg%06dl\n" % i)
        f.write(memoryview(hb[int(o):int(o) + int(L)]))
        f.write(b"\n")
PY
# run <binary> <sub> [stdout file]: the wall time in $T; any exit status but 0 ends the script (nothing more is started on the device)
run() {
  local t0=$(date +%s.%N)
  if ! timeout -k 10 120 env $EXTRA "$1" "$2" /dev/shm/asm1.fa > "${3:-/dev/null}" 2> /dev/shm/err.txt; then
    echo "$1 $2 failed" >&2; tail -5 /dev/shm/err.txt >&2; rm -f /dev/shm/asm1.fa /dev/shm/out.a /dev/shm/out.b; exit 1
  fi
  T=$(python3 -c "import time; print('%.3f' % (time.time() - $t0))")
}
stats() { python3 -c "import sys; v = sorted(map(float, sys.argv[1:])); print('median %.3f s, range %.3f-%.3f s, n %d' % ((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, v[0], v[-1], len(v)))" "$@"; }
for sub in sdust telofind; do
  ta=""; tb=""
  run "$A" $sub /dev/shm/out.a; run "$B" $sub /dev/shm/out.b
  echo "$sub md5 A $(md5sum < /dev/shm/out.a | cut -c1-12) B $(md5sum < /dev/shm/out.b | cut -c1-12)"
  for rep in $(seq $N); do
    run "$A" $sub; ta="$ta $T"
    run "$B" $sub; tb="$tb $T"
  done
  echo "$sub A ($A): $(stats $ta) |$ta"
  echo "$sub B ($B): $(stats $tb) |$tb"
  if [ -n "$PIECES" ]; then EXTRA=CORNETTO_CLI_WHOLE=0 run "$B" $sub; echo "$sub B CORNETTO_CLI_WHOLE=0: $T s"; fi
done
rm -f /dev/shm/asm1.fa /dev/shm/out.a /dev/shm/out.b /dev/shm/err.txt
