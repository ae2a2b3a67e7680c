"""The ungapped stage's registers, scratch and LDS, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_seed_resources.py reads it).  CPU-only; skipped without hipcc.

Why: search_ungapped_kernel is one wave per candidate over some two million candidates, and a spill or a trip to scratch memory
would sit inside its 64-cell step.  Its LDS is the score table of 21 rows of 32 bytes and nothing else: the two scans of a step
are shuffles.  The join's instantiation keeps its runs' targets in device memory, so its tile is two arrays of 2048 words, not
three: eight waves per SIMD where the plain join has six."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["search_join_diag_kernel", "ungapped_best_kernel", "ungapped_cand_kernel", "search_ungapped_kernel", "ungapped_keep_kernel",
           "ungapped_emit_kernel", "ungapped_top_emit_kernel", "ungapped_place_kernel"]
TABLE, TILE = 21 * 32, 2048


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_eight_waves_per_simd(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)
    assert r["vgprs"] <= 64 and r["occupancy"] >= 8, (kernel, r)


def test_the_lds_is_the_score_table_and_the_join_s_tile():
    res = kr.resources()
    assert res["search_ungapped_kernel"]["lds"] == TABLE
    assert res["search_join_diag_kernel"]["lds"] == 2 * 4 * TILE
    assert all(res[k]["lds"] == 0 for k in KERNELS if k not in ("search_ungapped_kernel", "search_join_diag_kernel"))
