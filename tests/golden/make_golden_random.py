#!/usr/bin/env python3
"""Record the reference's outputs on the random cases of the differential tests of tests/test_oracle_golden.py, so that those
tests run where oracle/_ref is not built.  Needs oracle/_ref (`make -f oracle/ref.mk`) and oracle/liboracle.so (`make -C oracle`).
Inputs and outputs go into the fixture together, so the tests do not depend on numpy's bit stream.

    python tests/golden/make_golden_random.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_bind as ob  # noqa: E402
from helpers import fastx_random_texts, pack_bytes, ref_sdust, sdust_random_cases, seq_prints_records  # noqa: E402

REFSO = os.path.join(ROOT, "oracle", "_ref", "libcornetto_ref.so")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "cornetto")


def main():
    if not (os.path.exists(REFSO) and os.path.exists(REFBIN)):
        sys.exit("build the reference first: make -f oracle/ref.mk")
    cases = sdust_random_cases()
    ivls = ref_sdust(REFSO, cases)
    seqs, seq_offs, _ = pack_bytes([s for s, _, _ in cases])
    iv_offs = np.zeros(len(ivls) + 1, dtype=np.int64)
    iv_offs[1:] = np.cumsum([len(x) for x in ivls])
    np.savez_compressed(os.path.join(HERE, "ref_sdust_random.npz"), seqs=seqs, seq_offs=seq_offs,
                        T=np.array([t for _, t, _ in cases], dtype=np.int32), W=np.array([w for _, _, w in cases], dtype=np.int32),
                        ivls=np.concatenate(ivls), ivl_offs=iv_offs)

    texts = fastx_random_texts()
    fa2bed, seq = [], []
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "t.fq")
        for text in texts:
            open(f, "wb").write(text)
            recs, rc = ob.fastx_parse(text)
            fa2bed.append(subprocess.run([REFBIN, "fa2bed", f], capture_output=True).stdout)
            seq.append(subprocess.run([REFBIN, "seq", "-m", "0", f], capture_output=True).stdout if seq_prints_records(text, recs, rc) else None)
    t, t_offs, _ = pack_bytes(texts)
    a, a_offs, _ = pack_bytes(fa2bed)
    q, q_offs, q_present = pack_bytes(seq)
    np.savez_compressed(os.path.join(HERE, "ref_fastx_random.npz"), texts=t, text_offs=t_offs, fa2bed=a, fa2bed_offs=a_offs,
                        seq=q, seq_offs=q_offs, seq_present=q_present)


if __name__ == "__main__":
    main()
