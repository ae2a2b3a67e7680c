"""The registers of the kernels behind the ops, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_trace_resources.py reads it).  CPU-only; skipped without hipcc.

Why: trace_columns_kernel is trace_pairs_kernel with the walk's columns recorded.  The walk is wave-uniform and its state lives in
scalar registers, of which trace_pairs_kernel<true> leaves two free: the recording keeps its own state in vector registers and
reads its arguments behind one pointer, and a spill would put memory on every move of the walk."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["trace_columns_kernel<false>", "trace_columns_kernel<true>", "ops_fill_kernel", "ops_starts_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


@pytest.mark.parametrize("long", ["false", "true"])
def test_the_recording_kernel_has_its_twins_lds_and_occupancy(long):
    res = kr.resources()
    mine, twin = res["trace_columns_kernel<%s>" % long], res["trace_pairs_kernel<%s>" % long]
    assert mine["lds"] == twin["lds"] and mine["occupancy"] == twin["occupancy"], (mine, twin)
    assert mine["vgprs"] <= 64                           # eight waves per SIMD by registers, as the twin


def test_the_fill_kernel_uses_no_lds_and_runs_at_full_occupancy():
    r = kr.resources()["ops_fill_kernel"]
    assert r["lds"] == 0 and r["occupancy"] == 8, r
