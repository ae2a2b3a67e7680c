"""The resident search's kernels' registers, scratch and LDS, from the compiler's own resource report (tools/kernel_resources.py,
as tests/test_band_resources.py reads it).  CPU-only; skipped without hipcc.

Why: the probe is a dependent chain of loads, one per level of its search, and a spill would put scratch memory on it; the
two-source join kernels keep the one-batch join's tile, and with a third run array in LDS they must still fit the workgroups per
CU the one-batch join has: wx and the two first pairs of a run are 3 * 2048 words, its 24 576 B."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["searchdb_kmers_kernel", "searchdb_masked_kernel", "searchdb_probe_kernel", "searchdb_run_compact_kernel",
           "searchdb_join_kernel", "searchdb_join_diag_kernel"]
JOIN_LDS = 3 * 2048 * 4


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)
    assert r["vgprs"] <= 64, (kernel, r)


def test_the_two_source_joins_lds_is_at_most_the_one_batch_join_s():
    res = kr.resources()
    assert res["search_join_kernel"]["lds"] == JOIN_LDS == 24576
    for kernel in ("searchdb_join_kernel", "searchdb_join_diag_kernel"):
        assert res[kernel]["lds"] <= JOIN_LDS and res[kernel]["occupancy"] >= res["search_join_kernel"]["occupancy"], (kernel, res[kernel])
    for kernel in KERNELS[:4]:
        assert res[kernel]["lds"] == 0, kernel
