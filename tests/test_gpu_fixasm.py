"""GPU: `cornetto fixasm` on the device path (framing on the device, the output text written by the emit kernel, cornetto_amd/csrc/emit.hip)
against the same recorded outputs, restatement and reference binary as the host path (tests/test_fixasm_host.py); small pieces and windows so
that records straddle both; FASTQ input; CORNETTO_DEVICES; one case of about 300 Mbases against the reference by sha256; and the Python
method over the C ABI (cornetto_emit_*) against a numpy restatement of reverse_complement() (src/fixasm.c:208-224)."""
import hashlib
import os
import random

import numpy as np
import pytest

import cornetto_amd
import fixasm_cases as fc

pytestmark = pytest.mark.gpu

SMALL = {"CORNETTO_FASTQ_PIECE": "4096", "CORNETTO_EMIT_SLAB": "1000"}


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(cornetto_amd.CLI_PATH), "build the CLI first (make -C cornetto_amd)"
    return cornetto_amd.CLI_PATH


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return fc.golden_inputs(str(tmp_path_factory.mktemp("fixasm_in")))


@pytest.mark.parametrize("env", [{}, SMALL, {"CORNETTO_EMIT_SLAB": "17"}, {"CORNETTO_DEVICES": "0,0"}, {"CORNETTO_CLI_WHOLE": "0"}],
                         ids=["default", "small_pieces", "slab17", "devices", "pieces"])
@pytest.mark.parametrize("case,argv", fc.GOLDEN_CASES, ids=[c[0] for c in fc.GOLDEN_CASES])
def test_recorded_case(cli, inputs, tmp_path, case, argv, env):
    fc.same(fc.run_case(cli, argv, inputs, str(tmp_path), env), fc.load_golden(case))


@pytest.mark.parametrize("seed", range(200))
def test_random_case(cli, tmp_path, seed):
    fc.check_random(cli, 1000 + seed, str(tmp_path))


@pytest.mark.parametrize("seed", range(40))
def test_random_case_small_pieces_and_windows(cli, tmp_path, seed):
    """pieces of 4 kB and windows of 1000 bytes: records cross both, and contigs of up to 20 kb are longer than a window"""
    fc.check_random(cli, 5000 + seed, str(tmp_path), SMALL, big=True)


@pytest.mark.parametrize("seed", range(20))
def test_random_fastq(cli, tmp_path, seed):
    fc.check_random(cli, 9000 + seed, str(tmp_path), SMALL if seed % 2 else {}, fastq=True)


def _rc(seq):
    return seq[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def test_large_assembly_against_the_reference(cli, tmp_path):
    """about 300 Mbases in 60 contigs, 80-column lines, half of them reversed: sha256 of every output equals the reference's (or the
    restatement's where the reference binary is not built)"""
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTacgtN", dtype=np.uint8)
    lens = rng.integers(1_000_000, 9_000_000, size=60)
    lens[0] = 0
    recs = [("ctg%02d" % i, alphabet[rng.integers(0, alphabet.size, size=int(n))].tobytes()) for i, n in enumerate(lens)]
    fa = tmp_path / "big.fa"
    with open(fa, "wb") as fh:
        for name, s in recs:
            fh.write(b">" + name.encode() + b"\n")
            for i in range(0, len(s), 80):
                fh.write(s[i:i + 80] + b"\n")
            if not s:
                fh.write(b"\n")
    paf = "".join("%s\t%d\t0\t%d\t%s\tchr%d\t10\t0\t%d\t1\t1\t60\n" % (name, len(s), len(s), "+-"[i % 2], i % 7, 100 + i)
                  for i, (name, s) in enumerate(recs) if i != 5)
    (tmp_path / "big.paf").write_text(paf)
    argv = ["fixasm", "-r", "{R}", "-m", "{M}", "-w", "{W}", str(fa), str(tmp_path / "big.paf")]
    got = fc.run_case(cli, argv, {}, str(tmp_path))
    assert got["rc"] == 0, got["err"][-2000:]
    if os.path.exists(fc.REF_CLI):
        exp = fc.run_case(fc.REF_CLI, argv, {}, str(tmp_path))
    else:
        out, report, missing, wpaf, summ = fc.model(recs, paf)
        exp = {"rc": 0, "out": out, "report": report, "missing": missing, "wpaf": wpaf, "summary": summ}
    for k in ("out", "report", "missing", "wpaf"):
        g, e = got[k], exp[k]
        g, e = (g if isinstance(g, bytes) else g.encode()), (e if isinstance(e, bytes) else e.encode())
        assert hashlib.sha256(g).hexdigest() == hashlib.sha256(e).hexdigest(), k
    assert got["summary"] == exp["summary"]


def test_the_device_path_is_taken(cli, inputs, tmp_path):
    """CORNETTO_DEVICE names a device that does not exist: the device path fails (no silent host fallback)"""
    got = fc.run_case(cli, ["fixasm", "dup.fa", "dup.paf"], inputs, str(tmp_path), {"CORNETTO_DEVICE": "999"})
    assert got["rc"] == 1 and got["out"] == b"" and b"cannot open HIP device" in got["err"]


@pytest.mark.parametrize("seed", range(6))
def test_emit_windows_of_the_abi(seed):
    """random sequences, rc flags and header lengths; windows of zero length, unaligned, crossing records, the last byte"""
    rng = random.Random(seed)
    acc = cornetto_amd.Accel(0)
    try:
        letters = b"ACGTacgtNRYKM-ACGT"
        seqs = [bytes(rng.choice(letters) for _ in range(rng.choice([0, 1, 15, 16, 17, 63, 64, 65, rng.randint(0, 5000)])))
                for _ in range(rng.randint(1, 40))]
        asm = acc.asm_upload(seqs)
        recs, heads, exp = [], b"", []
        for _ in range(rng.randint(1, 60)):
            c = rng.randrange(len(seqs))
            rc = rng.random() < 0.5
            h = bytes(rng.choice(b"abcdefgh_0123>") for _ in range(rng.choice([0, 1, 2, rng.randint(0, 40)])))
            recs.append((c, int(rc), len(heads), len(h)))
            heads += h
            exp.append(h + (_rc(seqs[c]) if rc else seqs[c]) + b"\n")
        text = b"".join(exp)
        T = len(text)
        wins = [(0, 0), (T, 0), (T - 1, 1), (0, T)]
        for _ in range(30):
            a = rng.randrange(T)
            wins.append((a, rng.randint(0, T - a)))
        wins += [(a, min(4096 + 13, T - a)) for a in range(0, T, 4096 + 13)]
        total, got = acc.emit(asm, recs, heads, wins)
        assert total == T
        for (a, n), g in zip(wins, got):
            assert g == text[a:a + n], (a, n)
        asm.close()
    finally:
        acc.close()


def test_emit_rejects_bad_arguments():
    acc = cornetto_amd.Accel(0)
    try:
        asm = acc.asm_upload([b"ACGT"])
        with pytest.raises(cornetto_amd.AccelError):
            acc.emit(asm, [(1, 0, 0, 0)], b"", [])          # no contig 1
        with pytest.raises(cornetto_amd.AccelError):
            acc.emit(asm, [(0, 0, 0, 5)], b">a\n", [])      # header past the head bytes
        with pytest.raises(cornetto_amd.AccelError):
            acc.emit(asm, [(0, 0, 0, 0)], b"", [(0, 6)])     # window past the text (5 bytes)
        asm.close()
    finally:
        acc.close()
