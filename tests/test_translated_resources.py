"""The registers, scratch and LDS of the CALL stage's two kernels (kg_evidence.hpp), from the compiler's own resource report
(tools/kernel_resources.py, as tests/test_searchdb_resources.py reads it).  CPU-only; skipped without hipcc.

Why: both kernels are one record per lane with nothing to keep between records, so any scratch or spill would be the compiler's
accident, and a VGPR count above 32 would say that a whole 40-byte record is held where three of its fields are needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")


@pytest.mark.parametrize("kernel", ["evidence_flag_kernel", "evidence_emit_kernel"])
def test_no_spills_no_scratch_no_lds(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0 and r["lds"] == 0, (kernel, r)
    assert r["vgprs"] <= 32 and r["occupancy"] == 8, (kernel, r)
