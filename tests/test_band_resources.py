"""The banded kernels' registers, scratch and LDS, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_ungapped_resources.py reads it).  CPU-only; skipped without hipcc.

Why: align_band_kernel keeps align_pairs_kernel's cell state in registers for 64 steps at a time and adds the window's bounds;
the banded trace variants add the band's two values to a pass that has no scalar register to spare.  A spill of either kind
would put memory on the recurrence's chain.  The band kernel's LDS is the score table of 21 rows of 32 bytes and a carry of
2 * 256 + 64 columns of 8 bytes: smaller than align_pairs_kernel<false>'s, so more waves fit a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["align_band_kernel", "trace_band_kernel<false>", "trace_band_kernel<true>", "trace_band_columns_kernel<false>",
           "trace_band_columns_kernel<true>"]
TABLE, CARRY = 21 * 32, 8 * (2 * 256 + 64)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_at_most_64_vgprs(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)
    assert r["vgprs"] <= 64, (kernel, r)


def test_the_band_kernel_s_lds_is_the_table_and_the_carry():
    res = kr.resources()
    assert res["align_band_kernel"]["lds"] == TABLE + CARRY < res["align_pairs_kernel<false>"]["lds"]
    assert res["align_band_kernel"]["occupancy"] == 8


def test_the_banded_trace_variants_keep_the_plain_ones_lds_and_occupancy():
    res = kr.resources()
    for long_ in ("false", "true"):
        for plain, band in (("trace_pairs_kernel", "trace_band_kernel"), ("trace_columns_kernel", "trace_band_columns_kernel")):
            a, b = res["%s<%s>" % (plain, long_)], res["%s<%s>" % (band, long_)]
            assert a["lds"] == b["lds"] and a["occupancy"] == b["occupancy"], (plain, long_, a, b)
