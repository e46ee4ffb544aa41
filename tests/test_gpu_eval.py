"""GPU: `cornetto nx | report | telocontigs | asmstats` on the device path (FASTA/FASTQ framed on the device, names and lengths only):
every recorded case against the outputs recorded from the reference, with the whole-file text (default), the piece loop
(CORNETTO_CLI_WHOLE=0) and pieces of 4 KiB that records straddle (CORNETTO_FASTQ_PIECE=4096); plain, gz and FASTQ inputs and a FASTA that
stops being plain partway through are among the fixtures.  `report` over many files opens the device once.  One assembly of about 300
Mbases gives the same stdout (sha256) on the device path as on the host path, and as the reference binary where it is built."""
import hashlib
import os

import numpy as np
import pytest

import cornetto_amd
import eval_cases as ec
from cornetto_amd import synth

pytestmark = pytest.mark.gpu

HOST = {"CORNETTO_ACCEL": "no", "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eval_in"))
    return ec.golden_inputs(d)


@pytest.mark.parametrize("env", [{}, {"CORNETTO_CLI_WHOLE": "0"}, {"CORNETTO_FASTQ_PIECE": "4096"}], ids=["whole", "pieces", "small_pieces"])
@pytest.mark.parametrize("case,argv", ec.GOLDEN_CASES, ids=[c[0] for c in ec.GOLDEN_CASES])
def test_recorded_case(cli, inputs, tmp_path, case, argv, env):
    ec.same(ec.run_case(cli, argv, inputs, str(tmp_path), env), ec.load_golden(case), inputs)


def test_report_over_many_files_opens_the_device_once(cli, inputs, tmp_path):
    files = ["asm.fa", "asm.fa.gz", "reads.fq", "reads.fq.gz", "mixed.fa", "mixed.fa.gz", "many.fa", "allempty.fa", "empty.fa", "ref.fa"]
    argv = ["report"] + files * 2
    got = ec.run_case(cli, argv, inputs, str(tmp_path), {"CORNETTO_CLI_TRACE": "1"})
    exp = ec.run_case(cli, argv, inputs, str(tmp_path), HOST)
    assert got["rc"] == 0 and got["out"] == exp["out"], got["err"][-2000:]
    opened = [ln for ln in got["err"].decode(errors="replace").splitlines() if ln.startswith("[cli trace] device") and "opened" in ln]
    assert len(opened) == 1, opened


def test_the_device_path_is_taken(cli, inputs, tmp_path):
    """CORNETTO_DEVICE names a device that does not exist: the device path fails (no silent host fallback)"""
    got = ec.run_case(cli, ["nx", "asm.fa"], inputs, str(tmp_path), {"CORNETTO_DEVICE": "999"})
    assert got["rc"] == 1 and got["out"] == b"" and b"cannot open HIP device" in got["err"]


def test_large_assembly(cli, tmp_path):
    """about 300 Mbases in 100 contigs of hifiasm-like lengths (synth.contig_lengths), 80-column lines: every sub-command prints the same
    bytes on the device path as on the host path, and as the reference binary where it is built"""
    lens = synth.contig_lengths(300_000_000)
    assert len(lens) <= 100            # (telocontigs: where the reference's counts are defined)
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8)
    fa = tmp_path / "big.fa"
    names = ["ctg%03d" % i for i in range(len(lens))]
    with open(fa, "wb") as fh:
        for name, n in zip(names, lens):
            s = alphabet[rng.integers(0, alphabet.size, size=int(n))].tobytes()
            fh.write(b">" + name.encode() + b" synthetic\n")
            fh.write(b"\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + b"\n")
    bed = "".join("%s\t0\t%d\n" % (names[i], 1000) for i in range(0, len(names), 3)) + "%s\t5\t900\n" % names[1]
    (tmp_path / "big.bed").write_text(bed)
    # asmstats -s big.fa: the assembly's own records are the chromosome list (the multi-GB input of the documented workflow)
    report = "".join("q%d\t%s\n" % (i, names[i % 9]) for i in range(30))
    paf = "".join("q%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t10\t10\t60\n" % (i, 50000 + i, 1000, names[(i * 5) % 9], lens[(i * 5) % 9], i * 1000,
                                                                        i * 1000 + 150000 * (i % 4)) for i in range(30))
    (tmp_path / "q.tsv").write_text(report)
    (tmp_path / "q.paf").write_text(paf)
    qbed = "".join("q%d\t0\t10\n" % i for i in range(0, 30, 2)) + "q4\t20\t30\n"
    (tmp_path / "q.bed").write_text(qbed)
    for argv in (["nx", str(fa)], ["nx", "-g", "3.1G", str(fa)], ["report", str(fa), str(fa)], ["telocontigs", str(fa), str(tmp_path / "big.bed")],
                 ["asmstats", "-s", str(fa), str(tmp_path / "q.paf"), str(tmp_path / "q.bed"), "-r", str(tmp_path / "q.tsv")]):
        got = ec.run_case(cli, argv, {}, str(tmp_path))
        host = ec.run_case(cli, argv, {}, str(tmp_path), HOST)
        assert got["rc"] == 0 and host["rc"] == 0, (argv, got["err"][-2000:], host["err"][-2000:])
        assert hashlib.sha256(got["out"]).hexdigest() == hashlib.sha256(host["out"]).hexdigest(), argv
        if os.path.exists(ec.REF_CLI):
            ref = ec.run_case(ec.REF_CLI, argv, {}, str(tmp_path))
            assert ref["rc"] == 0 and hashlib.sha256(got["out"]).hexdigest() == hashlib.sha256(ref["out"]).hexdigest(), argv
