"""Time of the frameshift repair on the GPU (kg_regionset_repair), one JSON line per measurement and one summary line per input.

    python tools/repair_time.py [--reps 8] [--regions 1000000] [--out profiles/repair_time.jsonl]

Inputs:
  planted    the contigs of tests/test_orfs_host.planted_orf_contigs (every third gene with a deleted base), scanned with their
             own table; the repair gets the result's device CALLs (kg_result_repair).
  two_frame  --regions contigs of 90 nucleotides, each one two-frame region of two CALLs (the first chain of
             tests/repair_cases.py), as caller-held lists (kg_regions_calls): every region is a candidate and is repaired.
Per input and repetition:
  orfs    the yardstick of the same run: kg_regionset_orfs on the same batch, device ms (kg_orf_stats) and wall ms.
  repair  kg_regionset_repair on that ORF set: device ms (kg_repair_stats: the planes again, two sorts of the CALLs, the checks,
          the chain, the proteins) and wall ms (the call has two host waits), and the counts.
The first repetition of an input carries the module load or the first allocations of its size: the summary leaves it out and
gives the median, the smallest and the largest of the others.  No ratio is fixed in advance.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from coding_time import _emit  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402


def _mid(values) -> dict:
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def two_frame_regions(n: int):
    """n copies of the deletion chain of tests/repair_cases.py on the '+' strand -> (calls, bytes, offsets)."""
    import repair_cases as RC
    case = RC.cases()[0]
    seq = np.tile(np.frombuffer(case["text"], dtype=np.uint8), n)
    off = np.arange(n + 1, dtype=np.int64) * RC.L
    calls = np.zeros(2 * n, dtype=N.CALL_DTYPE)
    for k, (f, a, z, cnt) in enumerate(case["calls"]):
        part = calls[k::2]
        part["container"], part["start"], part["end"], part["count"], part["fI"], part["weightedHits"] = 6 * np.arange(n) + f, a, z, cnt, 7, 1.0
    return calls, seq, off


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--regions", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_time.jsonl"))
    a = ap.parse_args()
    import torch
    import test_orfs_host as HO
    gpu = torch.cuda.get_device_name(0)
    lib = N.load()
    img, dna, poff, _ = HO.planted_orf_contigs()
    inputs = [("planted", None, np.frombuffer(dna, dtype=np.uint8), poff), ("two_frame",) + two_frame_regions(a.regions)]
    rp, op = N.KgRepairParams(7, 0, 4, 0), N.KgOrfParams(7, 1, 0)
    with hotpath.SignatureTable.from_bytes(img, 0) as tab:
        for name, calls, seq, off in inputs:
            batch = (seq.ctypes.data, 0, off.ctypes.data, len(off) - 1)
            result = tab.scan(seq, off, hotpath.Params(min_hits=4)) if calls is None else None
            kept = {"orfs_ms": [], "orfs_wall_ms": [], "repair_ms": [], "repair_wall_ms": []}
            try:
                for rep in range(a.reps):
                    rh, oh, new = C.c_void_p(), C.c_void_p(), C.c_void_p()
                    try:
                        if calls is None:
                            N.check(lib.kg_result_regions(result._h, C.byref(N.KgRegionParams(300, 12, 100)), off.ctypes.data, C.byref(rh)))
                        else:
                            N.check(lib.kg_regions_calls(0, C.byref(N.KgRegionParams(600, 0, 0)), calls.ctypes.data, calls.size, off.ctypes.data,
                                                         len(off) - 1, C.byref(rh)))
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        N.check(lib.kg_regionset_orfs(rh, C.byref(op), *batch, C.byref(oh)))
                        wall_orfs = (time.perf_counter() - t0) * 1e3
                        ost = N.KgOrfStats()
                        N.check(lib.kg_orfset_stats(oh, C.byref(ost)))
                        t0 = time.perf_counter()
                        if calls is None:
                            N.check(lib.kg_result_repair(result._h, rh, oh, C.byref(rp), *batch, C.byref(new)))
                        else:
                            N.check(lib.kg_regionset_repair(rh, oh, calls.ctypes.data, 0, calls.size, C.byref(rp), *batch, C.byref(new)))
                        wall = (time.perf_counter() - t0) * 1e3
                        st = N.KgRepairStats()
                        N.check(lib.kg_orfset_junctions_stats(new, C.byref(st)))
                    finally:
                        for h, free in ((new, lib.kg_orfset_free), (oh, lib.kg_orfset_free), (rh, lib.kg_regionset_free)):
                            if h.value:
                                free(h)
                    base = {"input": name, "contigs": len(off) - 1, "nucleotides": int(off[-1]), "regions": int(ost.orfs), "gpu": gpu, "rep": rep}
                    _emit(a.out, dict(base, what="orfs", device_ms=round(ost.ms, 3), wall_ms=round(wall_orfs, 2)))
                    d = st.as_dict()
                    ms = d.pop("ms")
                    _emit(a.out, dict(base, what="repair", device_ms=round(ms, 3), wall_ms=round(wall, 2), repair_over_orfs=round(ms / ost.ms, 3), **d))
                    if rep > 0:
                        for key, v in (("orfs_ms", ost.ms), ("orfs_wall_ms", wall_orfs), ("repair_ms", ms), ("repair_wall_ms", wall)):
                            kept[key].append(v)
            finally:
                if result is not None:
                    result.close()
            if kept["repair_ms"]:
                _emit(a.out, dict({"input": name, "contigs": len(off) - 1, "nucleotides": int(off[-1]), "gpu": gpu}, what="summary",
                                  reps=len(kept["repair_ms"]), **{k: _mid(v) for k, v in kept.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
