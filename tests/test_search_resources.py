"""The search kernels' registers and LDS, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_kernel_resources.py reads it).  CPU-only; skipped without hipcc.

Why: the join writes one key per (query, target) of every shared k-mer, the most items of the whole call; a spill would put a
trip to scratch memory into the loop that places them.  Its LDS is the tile's three run arrays and nothing else, which is what
bounds it whatever the input."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["search_init_kernel", "search_kmer_heads_kernel", "search_run_weights_kernel", "search_run_compact_kernel",
           "search_join_kernel", "search_cand_flags_kernel", "search_cand_emit_kernel", "search_query_heads_kernel",
           "search_top_flags_kernel", "search_top_emit_kernel", "search_order_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_the_lds_is_the_joins_tile():
    from kmergutsjava_amd import _native as N
    res = kr.resources()
    assert res["search_join_kernel"]["lds"] == 3 * 4 * N.SEARCH_TILE
    assert all(res[k]["lds"] == 0 for k in KERNELS if k != "search_join_kernel")
    assert res["search_join_kernel"]["vgprs"] <= 64 and res["search_order_kernel"]["vgprs"] <= 64      # eight waves per SIMD
