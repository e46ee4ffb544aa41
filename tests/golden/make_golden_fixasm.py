"""Record the expected outputs of the `cornetto fixasm` cases of tests/fixasm_cases.py (GOLDEN_CASES) from the UNMODIFIED reference
binary (oracle/_ref/cornetto, built by `make -f oracle/ref.mk`) into tests/golden/fixasm/: <case>.json (exit status, the three count
lines of stderr, -r / -m / -w files, the name of the stdout file) and out_<sha256 prefix>.gz (stdout; cases with the same stdout share it).  Run from the repository root:

    python tests/golden/make_golden_fixasm.py
"""
import glob
import gzip
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fixasm_cases as fc  # noqa: E402


def main():
    assert os.path.exists(fc.REF_CLI), "build the reference first: make -f oracle/ref.mk"
    os.makedirs(fc.FIX, exist_ok=True)
    for f in glob.glob(os.path.join(fc.FIX, "*")):
        os.remove(f)
    with tempfile.TemporaryDirectory() as d:
        inputs = fc.golden_inputs(d)
        for case, argv in fc.GOLDEN_CASES:
            got = fc.run_case(fc.REF_CLI, argv, inputs, d)
            rec = {k: got[k] for k in ("rc", "summary", "report", "missing", "wpaf")}
            rec["out_file"] = "out_%s.gz" % hashlib.sha256(got["out"]).hexdigest()[:12]
            json.dump(rec, open(os.path.join(fc.FIX, case + ".json"), "w"), indent=1, sort_keys=True)
            with open(os.path.join(fc.FIX, rec["out_file"]), "wb") as fh:
                fh.write(gzip.compress(got["out"], 9, mtime=0))
            print(case, rec["rc"], rec["summary"], len(got["out"]))


if __name__ == "__main__":
    main()
