"""GPU: bgzf_inflate over the hand-assembled deflate streams of tests/deflate_asm.py — what zlib's inflate accepts and zlib's deflate never
writes, and matches, literal runs and stored blocks at every position against the 64 lanes, the literal gather and the lazy fence, which
the CPU build of the decoder cannot check (its lanes run one after the other).  Every one of these streams went through the sanitizer
program first (tests/test_deflate_asm_host.py: inflate_sim --status under AddressSanitizer + UBSan, where the invalid ones get the
CNI_BAD_* reason aimed at).  The output is filled with 0xA5 beforehand and no data byte has that value: a byte read before its store
landed shows as 0xA5, and so does a write outside a block's range in the 64 bytes of canary between the blocks."""
import numpy as np
import pytest

import cornetto_amd
import deflate_asm as da

pytestmark = pytest.mark.gpu

VALID = da.valid_cases()
INVALID = da.invalid_cases()


@pytest.fixture(scope="module")
def acc():
    a = cornetto_amd.Accel(0)
    yield a
    a.close()


def _inflate(acc, chain):
    """the chain inflated with 64 bytes of canary in front of every block and 256 behind the text -> (bytes, first_bad, blocks)"""
    blocks, resume, broken = cornetto_amd.bgzf_scan(chain)
    assert resume == len(chain) and not broken
    blocks["dst"] += 64 * np.arange(1, len(blocks) + 1)
    got, first_bad = acc.bgzf_inflate(chain, blocks=blocks, fill=da.FILL)
    return got, first_bad, blocks


def _check(got, blocks, expected):
    """every block whose expected bytes are given holds them; every byte outside the blocks' ranges is the fill value"""
    free = np.ones(len(got), dtype=bool)
    for i, b in enumerate(blocks):
        d, n = int(b["dst"]), int(b["n_dst"])
        free[d:d + n] = False
        if expected[i] is not None:
            assert n == len(expected[i])
            if got[d:d + n] != expected[i]:
                at = next(k for k in range(n) if got[d + k] != expected[i][k])
                raise AssertionError("block %d differs from byte %d on: %r, zlib has %r" % (i, at, got[d + at:d + at + 16], expected[i][at:at + 16]))
    assert free.sum() == 64 * len(blocks) + 256 and bytes(np.frombuffer(got, dtype=np.uint8)[free]) == bytes([da.FILL]) * int(free.sum())


def _run_valid(acc, names):
    chain = b"".join(da.member_raw(VALID[n][0], VALID[n][1]) for n in names)
    got, first_bad, blocks = _inflate(acc, chain)
    assert first_bad == -1 and acc.last_status == 0 and len(blocks) == len(names)
    _check(got, blocks, [VALID[n][1] for n in names])


@pytest.mark.parametrize("name", da.singles())
def test_every_named_shape_inflates_to_zlibs_bytes(acc, name):
    _run_valid(acc, [name])


@pytest.mark.parametrize("grid", ("tiny_blocks",) + da.GROUPS)
def test_every_member_of_a_grid_inflates_to_zlibs_bytes(acc, grid):
    names = [grid] if grid == "tiny_blocks" else da.group(grid)
    assert len(names) == {"tiny_blocks": 1, "fence_grid": 20, "copy_grid": 255, "seeded": 300}[grid]
    _run_valid(acc, names)


@pytest.mark.parametrize("name", sorted(INVALID))
def test_an_invalid_stream_is_reported_and_writes_inside_its_own_range(acc, name):
    payload, n_dst, _ = INVALID[name]
    left, right = "fence_grid/k65_out1+1", "len258_as_284"
    chain = da.member_raw(VALID[left][0], VALID[left][1]) + da.member_raw(payload, isize=n_dst, crc=0) + da.member_raw(VALID[right][0], VALID[right][1])
    got, first_bad, blocks = _inflate(acc, chain)
    assert first_bad == 1 and acc.last_status == -6 and len(blocks) == 3 and int(blocks["n_dst"][1]) == n_dst
    _check(got, blocks, [VALID[left][1], None, VALID[right][1]])
