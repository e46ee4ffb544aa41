"""The planted inputs of tests/test_gpu_sdust_groups.py, checked without a device, for every group size the kernel is measured with: the
contig lengths are there, groups span contig borders, every seam feature lies at a carried and at a redone seam and is masked by the oracle,
the planted bytes make exactly the chunks unclean they are planted for, and the number of carried seams is the closed form (less the seams
named where bytes are planted).  Keeps the GPU module from silently losing its cases."""
import pytest

import group_cases as gc


@pytest.mark.parametrize("G", gc.GROUPS)
@pytest.mark.parametrize("T,W", gc.PAIRS)
def test_cases(T, W, G):
    k = gc.assembly(T, W, G)
    gc.check(k)
    gc.check(gc.assembly(T, W, G, dirty=False))
    assert max(len(s) for s in k.seqs) <= 12 * gc.CHUNK          # a few kbases per contig
    assert k.exp and len(gc.chunk_table(k.seqs)) > 3 * G


def test_closed_form_by_hand():
    """two contigs of 3 and 2 chunks, G = 2: table indices 0 1 2 | 3 4; carried: 1 (0 -> 1) and — 2 begins a group, 3 begins a contig — 4? no:
    4 begins a group.  G = 4: 1, 2 carried, 3 begins a contig, 4 begins a group"""
    import numpy as np
    seqs = [np.full(3 * gc.CHUNK, ord("A"), np.uint8), np.full(2 * gc.CHUNK - 7, ord("C"), np.uint8)]
    assert gc.carried(seqs, 2) == [1] and gc.closed_form(seqs, 2) == 1
    assert gc.carried(seqs, 4) == [1, 2] and gc.closed_form(seqs, 4) == 2
    assert gc.carried(seqs, 8) == [1, 2, 4] and gc.closed_form(seqs, 8) == 3
    seqs[0][gc.CHUNK + 5] = ord("N")                              # chunk 1 is walked: 0 -> 1 and 1 -> 2 are lost
    assert gc.carried(seqs, 8) == [4]
    seqs[0][gc.CHUNK + 5] = ord("A")
    seqs[0][2 * gc.CHUNK - 128] = ord("N")                        # the first byte of chunk 2's halo: 1 and 2 are walked
    assert gc.unclean(seqs) == [False, True, True, False, False] and gc.carried(seqs, 8) == [4]
