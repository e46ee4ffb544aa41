#!/usr/bin/env python3
"""Golden vectors for `cornetto telowin` on a hit list that telofind never writes (tests/telowin_cases.py: seam_contigs()) from the UNMODIFIED
reference binary (oracle/_ref/cornetto, built by `make -f oracle/ref.mk`).  Only where the reference's sources are; the input and the
expected outputs are committed.

    python tests/golden/make_golden_telowin_hits.py

`100 0`: every window the reference visits, with its count; `100 0.5`: the adjusted threshold is 0.5 itself; the other two as the other
telowin goldens."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "cornetto")
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import telowin_cases as twc  # noqa: E402

TSV = "hits_craft.telomere"
RUNS = [("100", "0", "hits_craft.i100t0.telowin.exp"), ("100", "0.5", "hits_craft.i100t05.telowin.exp"),
        ("99.9", "0.4", "hits_craft.telowin.exp"), ("90", "0.1", "hits_craft.i90t01.telowin.exp")]
LIMIT = 200_000            # bytes per committed file


if __name__ == "__main__":
    case = twc.seam_contigs()
    assert 0 in case["lens"] and len(set(case["names"])) < len(case["names"])
    with open(os.path.join(HERE, TSV), "wb") as f:
        f.write(twc.tsv(case))
    for identity, thr, out in RUNS:
        with open(os.path.join(HERE, out), "wb") as fo:
            rc = subprocess.run([REF, "telowin", os.path.join(HERE, TSV), identity, thr], stdout=fo, stderr=subprocess.DEVNULL).returncode
        assert rc == 0, (out, rc)
    for f in [TSV] + [r[2] for r in RUNS]:
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < LIMIT, (f, size)
        print(f, sum(1 for _ in open(os.path.join(HERE, f), "rb")), size)
