"""The seed window kernel's registers and LDS, from the compiler's own resource report (tools/kernel_resources.py, as
tests/test_search_resources.py reads it).  CPU-only; skipped without hipcc.

Why: the kernel walks up to four shapes of up to 32 care positions per block of windows, and a spill or a trip to scratch memory
would sit inside that walk.  Its LDS is the class table of 256 bytes, one row of 128 class codes per wave and, in the counting
instantiation, the workgroup's 8-byte sum: that is what bounds it whatever the seed set."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")
KERNELS = ["seed_windows_kernel<false>", "seed_windows_kernel<true>"]
WAVES_PER_WG, ROW, TABLE = 4, 128, 256


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_and_no_scratch(kernel):
    r = kr.resources()[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_the_lds_is_the_table_and_the_waves_rows():
    res = kr.resources()
    assert res["seed_windows_kernel<true>"]["lds"] == TABLE + WAVES_PER_WG * ROW
    assert res["seed_windows_kernel<false>"]["lds"] == TABLE + WAVES_PER_WG * ROW + 8
    assert all(res[k]["vgprs"] <= 64 for k in KERNELS)                  # eight waves per SIMD
