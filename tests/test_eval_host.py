"""CPU: `cornetto nx | report | telocontigs | asmstats` on the host path (CORNETTO_ACCEL=no, no visible GPU) against the outputs recorded
from the unmodified reference binary (tests/golden/eval/, tests/golden/make_golden_eval.py) and against that binary where it is built
(oracle/_ref/cornetto): stdout bytes and exit status.  The seeded random cases are checked against the restatement in tests/eval_cases.py
(and the reference where it is built)."""
import os

import pytest

import cornetto_amd
import eval_cases as ec

HOST = {"CORNETTO_ACCEL": "no", "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eval_in"))
    return ec.golden_inputs(d)


@pytest.mark.parametrize("case,argv", ec.GOLDEN_CASES, ids=[c[0] for c in ec.GOLDEN_CASES])
def test_recorded_case(cli, inputs, tmp_path, case, argv):
    got = ec.run_case(cli, argv, inputs, str(tmp_path), HOST)
    ec.same(got, ec.load_golden(case), inputs)
    if os.path.exists(ec.REF_CLI):
        ec.same(got, ec.run_case(ec.REF_CLI, argv, inputs, str(tmp_path)), inputs)


def test_the_restatement_matches_the_recorded_cases(inputs):
    """the Python model the random cases are held to gives what the reference gave on the fixtures"""
    def out(case):
        g = ec.load_golden(case)
        return g["rc"], g["out"]
    asm_lens = [r[1] for r in ec.ASM]
    assert out("nx_asm") == (0, ec.nx_text(asm_lens))
    assert out("nx_g") == (0, ec.nx_text(asm_lens, ec.parse_num("3.1k")))
    assert out("nx_g_round") == (0, ec.nx_text(asm_lens, ec.parse_num("1000.5")))
    assert out("nx_allempty") == (0, ec.nx_text([0, 0]))
    assert out("nx_empty") == (0, ec.nx_text([]))
    assert out("report_one") == (0, ec.report_text(["<asm.fa>"], {"<asm.fa>": asm_lens}))
    assert out("telo_asm") == ec.telocontigs_text([r[:2] for r in ec.ASM], ec.TEL_BED)
    assert out("telo_many") == ec.telocontigs_text(ec.MANY, ec.MANY_BED)
    kh = cornetto_amd.khash_str_order
    assert out("as_default") == ec.asmstats_text("<as.paf>", ec.AS_BED, ec.AS_REPORT, ec.AS_PAF, kh=kh)
    assert out("as_trim") == ec.asmstats_text("<as.paf>", ec.AS_BED, ec.AS_REPORT, ec.AS_PAF, trim=True, kh=kh)
    assert out("as_human2") == ec.asmstats_text("<as.paf>", ec.AS_BED, ec.AS_REPORT, ec.AS_PAF, "human2", kh=kh)
    ref_names = ["chr2", "chrX", "chr1", "chrM", "chr01", "chr10", "chr3"]
    assert out("as_ref") == ec.asmstats_text("<as.paf>", ec.AS_BED, ec.AS_REPORT, ec.AS_PAF, "file", ref_names=ref_names, kh=kh)
    assert out("as_report_nopaf") == ec.asmstats_text("<as.paf>", ec.AS_BED, ec.AS_REPORT + "ctgA\tchr9\n", ec.AS_PAF, kh=kh)


@pytest.mark.parametrize("kind", ["nx", "report", "telocontigs", "asmstats"])
@pytest.mark.parametrize("seed", range(200))
def test_random_case(cli, tmp_path, kind, seed):
    ec.check_random(cli, kind, 5000 + seed, str(tmp_path), HOST, cornetto_amd.khash_str_order)
