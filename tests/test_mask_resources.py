"""The mask kernels' registers and LDS, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_seed_resources.py reads it).  CPU-only; skipped without hipcc.

Why: the window kernel counts the 21 letters of a window in three registers of seven 8-bit fields and walks up to 32 positions per
lane; a spill or a trip to scratch memory would sit inside that walk, and an array of counters indexed by the letter would be
one.  Its LDS is one row of 128 letters per wave and the table of n * Lg(n) for n = 0..32 as 32-bit words: that is what bounds
it whatever the window.  The other passes use no LDS at all."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["mask_windows_kernel", "mask_runs_kernel", "mask_residues_kernel<false>", "mask_residues_kernel<true>", "mask_starts_kernel",
           "mask_apply_kernel"]
WAVES_PER_WG, ROW, TABLE = 4, 128, 33 * 4


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_the_lds_is_the_waves_rows_and_the_table():
    res = kr.resources()
    assert res["mask_windows_kernel"]["lds"] == WAVES_PER_WG * ROW + TABLE
    assert all(res[k]["lds"] == 0 for k in KERNELS[1:])
    assert all(res[k]["vgprs"] <= 64 for k in KERNELS)                  # eight waves per SIMD
