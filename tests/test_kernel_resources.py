"""Register budgets of the kernels the benchmark runs, from the compiler's own resource report (tools/kernel_resources.py: one
device-only compile, cached by source hash next to the built library).  CPU-only; skipped without hipcc.

Why these numbers (kg_partition.hpp, "Register budgets"): a scatter workgroup's four waves per SIMD and the index pass's four
share the SIMD's 512 VGPRs, 4 x 96 + 4 x 32; a spilled scalar register is a lane move plus hazard wait on the wave's issue
path, in kernels whose scalar stream is as long as their vector stream; scratch memory is a trip to HBM."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not found")

# the instantiations bench.py's flagship workload launches
SCATTER = "part_scatter_kernel<false,false,false>"
BENCH = [SCATTER, "bucket_index_kernel<4,1,true,false>", "verify_kernel<false,false,false>", "calls_wave_kernel",
         "hit_partition_kernel<true>", "hit_partition_kernel<false>", "group_place_kernel<false>"]


@pytest.fixture(scope="module")
def res():
    return kr.resources()


def test_the_bench_kernels_are_reported(res):
    for k in BENCH:
        assert k in res, (k, sorted(res))
        assert {"sgprs", "sgpr_spills", "vgprs", "vgpr_spills", "scratch", "occupancy"} <= set(res[k]), res[k]


@pytest.mark.parametrize("kernel", BENCH)
def test_no_spills_and_no_scratch(res, kernel):
    r = res[kernel]
    assert r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0 and r["scratch"] == 0, (kernel, r)


def test_scatter_and_index_share_a_simd(res):
    assert res[SCATTER]["vgprs"] <= 96 and res[SCATTER]["occupancy"] == 5, res[SCATTER]
    assert res["bucket_index_kernel<4,1,true,false>"]["vgprs"] <= 32, res["bucket_index_kernel<4,1,true,false>"]


def test_protein_scatter_has_no_scalar_spills(res):
    for k in ("part_scatter_kernel<true,false,false>", "part_scatter_kernel<true,true,false>", "part_scatter_kernel<true,true,true>"):
        assert res[k]["sgpr_spills"] == 0 and res[k]["scratch"] == 0, (k, res[k])


def test_touched_kernels_use_no_scratch(res):
    for k, r in res.items():
        if k.startswith(("part_scatter_kernel", "lowc_blocks_kernel", "calls_wave_kernel")):
            assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (k, r)
