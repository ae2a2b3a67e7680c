"""The alignment kernels' registers, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_kernel_resources.py reads it).  CPU-only; skipped without hipcc.

Why: the wave keeps a whole cell's state (H-left, E, what lane l + 1 reads, the diagonal, the residue, the next score, the
best) in registers for 64 steps at a time; a spill would put a trip to memory on every step of the recurrence's chain."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["align_pairs_kernel<false>", "align_pairs_kernel<true>", "align_cut_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_the_lds_is_the_table_and_the_carry():
    res = kr.resources()
    table = 21 * 32
    assert res["align_pairs_kernel<true>"]["lds"] in (table, table + 8)         # (its one-entry carry array is not used)
    assert res["align_pairs_kernel<false>"]["lds"] == 1024 * 8 + table and res["align_cut_kernel"]["lds"] == 0
    assert res["align_pairs_kernel<false>"]["vgprs"] <= 64         # eight waves per SIMD by registers; the LDS holds it to five
