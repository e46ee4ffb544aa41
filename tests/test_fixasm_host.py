"""CPU: `cornetto fixasm` on the host path (CORNETTO_ACCEL=no) against the unmodified reference binary where it is built
(oracle/_ref/cornetto) and against the outputs recorded from it (tests/golden/fixasm/, tests/golden/make_golden_fixasm.py): stdout, the -r / -m /
-w files, the three count lines on stderr and the exit status.  The seeded random cases are checked against the restatement in
tests/fixasm_cases.py (and the reference where it is built)."""
import os

import pytest

import cornetto_amd
import fixasm_cases as fc

HOST = {"CORNETTO_ACCEL": "no", "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fixasm_in"))
    return fc.golden_inputs(d)


@pytest.mark.parametrize("case,argv", fc.GOLDEN_CASES, ids=[c[0] for c in fc.GOLDEN_CASES])
def test_recorded_case(cli, inputs, tmp_path, case, argv):
    got = fc.run_case(cli, argv, inputs, str(tmp_path), HOST)
    fc.same(got, fc.load_golden(case))
    if os.path.exists(fc.REF_CLI):
        fc.same(got, fc.run_case(fc.REF_CLI, argv, inputs, str(tmp_path)))


def test_help_goes_to_stdout_with_h(cli, inputs, tmp_path):
    got = fc.run_case(cli, ["fixasm", "--help", "x"], inputs, str(tmp_path), HOST)
    assert got["rc"] == 1 and got["out"].startswith(b"Usage: cornetto fixasm <assembly.fa> <asm_to_ref.paf>\n")
    got = fc.run_case(cli, ["fixasm", "x"], inputs, str(tmp_path), HOST)
    assert got["rc"] == 1 and got["out"] == b"" and b"Usage: cornetto fixasm" in got["err"]


def test_the_restatement_matches_the_recorded_cases():
    """the Python model the random cases are held to gives what the reference gave on the fixtures"""
    from helpers import read_fastx
    recs = [(r[0].decode() if isinstance(r[0], bytes) else r[0], bytes(r[2])) for r in read_fastx(os.path.join(fc.GOLDEN, "mix.fa.gz"))]
    for case, trim in (("mix", False), ("mix_trim", True)):
        out, report, missing, wpaf, summ = fc.model(recs, fc.MIX_PAF, trim)
        exp = fc.load_golden(case)
        assert (out, report, missing, wpaf, summ) == (exp["out"], exp["report"], exp["missing"], exp["wpaf"], exp["summary"]), case


@pytest.mark.parametrize("seed", range(200))
def test_random_case(cli, tmp_path, seed):
    fc.check_random(cli, 1000 + seed, str(tmp_path), HOST)
