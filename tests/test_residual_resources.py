"""The registers, scratch and LDS of the residual stage's seven kernels (kg_residual.hpp), from the compiler's own resource report
(tools/kernel_resources.py, as tests/test_translated_resources.py reads it).  CPU-only; skipped without hipcc.

Why: every kernel is one record, one CALL or one 16-byte chunk per lane with a few words kept across a short loop, so any scratch
or spill would be the compiler's accident (the copy kernel's five dwords and four output words must stay in registers, not in a
runtime-indexed array in scratch), and a VGPR count above 32 would say that whole 48-byte records are held where a few of their
fields are needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")

KERNELS = ["residual_keys_kernel", "residual_mark_kernel", "residual_choose_kernel", "residual_layout_kernel", "residual_copy_kernel",
           "residual_keep_kernel", "residual_merge_kernel"]


def test_every_kernel_of_the_stage_is_listed():
    assert sorted(k for k in kr.resources() if k.startswith("residual_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_no_lds(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0 and r["lds"] == 0, (kernel, r)
    assert r["vgprs"] <= 32 and r["occupancy"] == 8, (kernel, r)
