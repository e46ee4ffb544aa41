"""Record the expected outputs of the `cornetto nx | report | telocontigs | asmstats` cases of tests/eval_cases.py (GOLDEN_CASES) from the
UNMODIFIED reference binary (oracle/_ref/cornetto, built by `make -f oracle/ref.mk`) into tests/golden/eval/<case>.json: the exit status and
stdout, with the paths of the fixture files written as <name>.  Run from the repository root:

    python tests/golden/make_golden_eval.py
"""
import glob
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import eval_cases as ec  # noqa: E402


def main():
    assert os.path.exists(ec.REF_CLI), "build the reference first: make -f oracle/ref.mk"
    os.makedirs(ec.EVAL, exist_ok=True)
    for f in glob.glob(os.path.join(ec.EVAL, "*.json")):
        os.remove(f)
    with tempfile.TemporaryDirectory() as d:
        inputs = ec.golden_inputs(d)
        for case, argv in ec.GOLDEN_CASES:
            got = ec.run_case(ec.REF_CLI, argv, inputs, d)
            rec = {"argv": argv, "rc": got["rc"], "out": ec.portable(got["out"], inputs).decode("latin-1")}
            json.dump(rec, open(os.path.join(ec.EVAL, case + ".json"), "w"), indent=1, sort_keys=True)
            print(case, rec["rc"], len(got["out"]))


if __name__ == "__main__":
    main()
