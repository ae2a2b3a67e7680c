"""tests/scan_model.py on the CPU: the two restatements of prefix_sum against the exact sum, and the record lengths of the limit
tests of test_gpu_orfs.py, test_gpu_coding.py and test_gpu_starts.py against both.

For every wrapping family the 32-bit chunk sums give a total below 2^32 while the items are 2^32 or more and some aligned chunk
wraps: with that total the stages did not refuse the call, which is what the GPU tests assert they do.  So each of those tests
fails when scan_partials_kernel goes back to 32-bit sums, and these assertions fail first when kScanChunk changes so that the
lists no longer wrap a chunk.  For the controls the three are the other way round: no chunk wraps and the wrapping scan's
total is the exact one -- 2^32, refused by either scan, for the list that straddles two chunks, and below 2^32 for the legal
list of the coding test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_model as SM  # noqa: E402

LIMIT = SM.LIMIT


def _same_mod(excl, exact):
    return [int(x) for x in excl] == [int(x) & 0xFFFFFFFF for x in exact]


def test_the_constants_are_the_kernels():
    assert SM.CHUNK == 2048 and SM.TOP == 256 and SM.N_LONG * SM.LONG == LIMIT
    # the families are built for a chunk that holds exactly the long records that make 2^32
    assert SM.N_LONG == SM.CHUNK


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 4096, 3 * 2048 + 5])
def test_small_lists_are_the_cumulative_sum_under_both_scans(n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 1000, size=n).astype(np.uint32)
    want = SM.scan_exact(lens)
    for scan in (SM.scan_wrapping, SM.scan_kernels):
        excl, total = scan(lens)
        assert total == want[1] and excl.dtype == np.uint32 and [int(x) for x in excl] == [int(x) for x in want[0]]
    assert not SM.chunk_wraps(lens)


def test_the_largest_items_the_total_is_exact_and_excl_is_the_prefix_modulo_2_32():
    """uint32 items at the top of their range: the total of the kernels is exact for any input, excl only modulo 2^32."""
    rng = np.random.default_rng(3)
    lens = rng.integers(0xF0000000, 0x100000000, size=2 * SM.CHUNK + 17, dtype=np.uint64).astype(np.uint32)
    want = SM.scan_exact(lens)
    excl, total = SM.scan_kernels(lens)
    assert total == want[1] > 2 ** 43 and _same_mod(excl, want[0]) and SM.chunk_wraps(lens)
    wexcl, wtotal = SM.scan_wrapping(lens)
    assert wtotal != want[1] and wtotal % LIMIT == want[1] % LIMIT and wexcl.tobytes() == excl.tobytes()


@pytest.mark.parametrize("short", [SM.SHORT_CODONS, 5, 6])         # the ORF stage's, the coding stage's, the start stage's
def test_the_limit_tests_lists_wrap_a_chunk_and_the_controls_do_not(short):
    fams = SM.families(short)
    assert sum(w for _, w in fams.values()) == 3 and len(fams) == 4
    for name, (lens, wraps) in fams.items():
        exact = SM.scan_exact(lens)[1]
        old = SM.scan_wrapping(lens)[1]
        new = SM.scan_kernels(lens)[1]
        assert new == exact >= LIMIT, name
        if wraps:
            assert old < LIMIT, name                    # the call was not refused
            assert SM.chunk_wraps(lens), name
        else:
            assert old == exact, name                   # refused by either scan
            assert not SM.chunk_wraps(lens), name
    assert SM.scan_wrapping(fams["chunk 0 is exactly 2^32"][0])[1] == 0
    assert SM.scan_exact(fams["chunk 1 wraps behind short records"][0])[1] == LIMIT + SM.N_LONG * short
    assert SM.scan_wrapping(fams["chunk 1 wraps behind short records"][0])[1] == SM.N_LONG * short
    assert SM.scan_exact(fams["control: two chunks of 2^31"][0])[1] == LIMIT


def test_the_legal_list_passes_the_sign_bit_inside_chunk_0():
    lens = SM.LEGAL
    exact = SM.scan_exact(lens)
    assert len(lens) == 1025 < SM.CHUNK and exact[1] == 2 ** 31 + 2 ** 21 < LIMIT and not SM.chunk_wraps(lens)
    for scan in (SM.scan_wrapping, SM.scan_kernels):
        excl, total = scan(lens)
        assert total == exact[1] and [int(x) for x in excl] == [int(x) for x in exact[0]]
    assert int(exact[0][-1]) == 2 ** 31 and int(exact[0][-2]) < 2 ** 31
