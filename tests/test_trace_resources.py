"""The traceback kernels' registers, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_align_resources.py reads it), and the alignment kernels' figures beside them: the new pass changes none.  CPU-only;
skipped without hipcc.

Why: the forward pass keeps align_pairs_kernel's cell state and a direction word in registers for 64 steps at a time, and the
walk is wave-uniform: its state lives in scalar registers.  A spill of either kind would put memory on the recurrence's chain or
on every move of the walk."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["trace_pairs_kernel<false>", "trace_pairs_kernel<true>"]
TABLE = 21 * 32


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_the_lds_is_the_table_and_the_carry_and_the_registers_hold_the_alignment_pass_occupancy():
    res = kr.resources()
    assert res["trace_pairs_kernel<true>"]["lds"] in (TABLE, TABLE + 8)         # (its one-entry carry array is not used)
    assert res["trace_pairs_kernel<false>"]["lds"] == 1024 * 8 + TABLE
    assert res["trace_pairs_kernel<false>"]["vgprs"] <= 64                       # eight waves per SIMD by registers; the LDS holds it to five
    assert res["trace_pairs_kernel<false>"]["occupancy"] == res["align_pairs_kernel<false>"]["occupancy"]


def test_the_alignment_kernels_figures_are_unchanged():
    """What the compiler reported for them before the traceback pass existed: the new kernels are separate
    functions in the same translation unit and change nothing in these."""
    res = kr.resources()
    want = {"align_pairs_kernel<false>": dict(sgprs=74, vgprs=58, lds=1024 * 8 + TABLE, occupancy=5),
            "align_pairs_kernel<true>": dict(sgprs=76, vgprs=56, occupancy=8), "align_cut_kernel": dict(lds=0)}
    for kernel, figures in want.items():
        r = res[kernel]
        assert {k: r[k] for k in figures} == figures and r["sgpr_spills"] == r["vgpr_spills"] == r["scratch"] == 0, (kernel, r)
