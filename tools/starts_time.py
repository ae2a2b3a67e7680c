"""Time of the start-codon choice on the GPU (kg_orfset_starts), one JSON line per measurement and one summary line per input.

    python tools/starts_time.py [--reps 12] [--out profiles/starts_time.jsonl]

Inputs: those of tools/coding_time.py -- the E. coli genome of tests/golden, eight copies of it as eight contigs, an all-A contig
of the genome's length (no codon is a start: one candidate per movable record) -- and an all-ATG contig of that length, the
worst case: frame 0 of '+' is one ORF whose every codon is a candidate with the same window.  The evidence ORFs are stood in for
as there (tools/coding_time.stand_in_regions).
Per input and repetition, on the set kg_orfset_add_free (min_res 100) gave:
  coding  the yardstick of the same run: kg_orfset_coding, training on its own records (min_train_pairs 0): count + score ms
          (kg_coding_stats) and wall ms.
  starts  kg_orfset_starts on the set coding gave, with the table of its counts, no region set (min_res 100 bounds every record),
          4 rounds, min_train_starts 0: count ms (the candidate list), choose ms (the rounds, the move, the proteins), wall ms
          -- the wall time carries the call's host waits: three for sizes and one per round --, and the counts.
The first repetition of an input carries the module load or the first allocations of its size: the summary leaves it out and
gives the median, the smallest and the largest of the others (a device window here is well below a millisecond on the genome,
so one repetition says little).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from coding_time import _emit, _offsets, stand_in_regions  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def _mid(values) -> dict:
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "starts_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    lib = N.load()
    genome = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))[1]
    total = sum(len(c) for c in genome)
    inputs = [("ecoli", genome, None), ("ecoli_x8", genome * 8, None), ("all_A", [b"A" * total], "one"),
              ("all_ATG", [(b"ATG" * (total // 3 + 1))[:total]], "one")]
    for name, contigs, how in inputs:
        off = _offsets(contigs)
        seq = np.frombuffer(b"".join(contigs), dtype=np.uint8)
        if how == "one":
            regs = np.zeros(1, dtype=N.REGION_DTYPE)
            regs[0] = (0, 0, 0, 32, 0, 10, 1.0, 1, 1, 0, 0, 1)
        else:
            regs = stand_in_regions(seq, off)
        base = {"input": name, "contigs": len(contigs), "nucleotides": int(off[-1]), "evidence": len(regs), "gpu": gpu}
        args = (seq.ctypes.data, 0, off.ctypes.data, len(off) - 1)
        kept = {"coding_ms": [], "coding_wall_ms": [], "count_ms": [], "choose_ms": [], "wall_ms": []}
        for rep in range(a.reps):
            hs = [C.c_void_p() for _ in range(4)]
            ev, both, scored, moved = hs
            try:
                N.check(lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, 1, 0)), regs.ctypes.data, len(regs), seq.ctypes.data, off.ctypes.data,
                                            len(off) - 1, C.byref(ev)))
                N.check(lib.kg_orfset_add_free(ev, C.byref(N.KgFreeParams(100, 7, 0)), *args, C.byref(both)))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                N.check(lib.kg_orfset_coding(both, C.byref(N.KgCodingParams(0, 0, 0)), None, *args, C.byref(scored)))
                wall_coding = (time.perf_counter() - t0) * 1e3
                cst, cm = N.KgCodingStats(), N.KgCodingModel()
                N.check(lib.kg_orfset_coding_stats(scored, C.byref(cst)))
                N.check(lib.kg_orfset_coding_model(scored, C.byref(cm)))
                T = hotpath.coding_table(np.array(cm.coding, dtype=np.int64), np.array(cm.background, dtype=np.int64))
                t0 = time.perf_counter()
                N.check(lib.kg_orfset_starts(scored, C.byref(N.KgStartParams(100, 7, 4, 0, 0)), T.ctypes.data, None, None, *args, C.byref(moved)))
                wall = (time.perf_counter() - t0) * 1e3
                st = N.KgStartStats()
                N.check(lib.kg_orfset_start_stats(moved, C.byref(st)))
            finally:
                for h in reversed(hs):
                    if h.value:
                        lib.kg_orfset_free(h)
            coding_ms = cst.ms_count + cst.ms_score
            _emit(a.out, dict(base, what="coding", rep=rep, device_ms=round(coding_ms, 3), wall_ms=round(wall_coding, 2)))
            d = st.as_dict()
            _emit(a.out, dict(base, what="starts", rep=rep, wall_ms=round(wall, 2), count_ms=round(d.pop("ms_count"), 3),
                              choose_ms=round(d.pop("ms_choose"), 3), starts_over_coding=round((st.ms_count + st.ms_choose) / coding_ms, 3), **d))
            if rep > 0:
                for key, v in (("coding_ms", coding_ms), ("coding_wall_ms", wall_coding), ("count_ms", st.ms_count), ("choose_ms", st.ms_choose),
                               ("wall_ms", wall)):
                    kept[key].append(v)
        if kept["wall_ms"]:
            _emit(a.out, dict(base, what="summary", reps=len(kept["wall_ms"]), **{k: _mid(v) for k, v in kept.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
