"""Time of the coding-potential filter on the GPU (kg_orfset_coding), one JSON line per measurement.

    python tools/coding_time.py [--reps 12] [--out profiles/coding_time.jsonl]

Inputs: the E. coli genome of tests/golden; eight copies of it, concatenated as eight contigs; an all-A contig of the genome's
length (every background count and every pair of its ORFs falls into one bin).  The fixture has no table, so the evidence ORFs
are stood in for by the genome's own six-frame ORFs of 300 residues: each is handed to kg_orfs_regions as a region of its own
extent (less the stop codon) and frame and comes back as a kept, not free, not interrupted record.  On the all-A contig one
region in frame 0 of '+' does the same.
Per input and repetition:
  add_free  the yardstick of the same run: kg_orfset_add_free (min_res 100) behind those records; it reads the batch once too.
            Device ms (kg_orf_stats.ms) and wall ms.
  coding    kg_orfset_coding on the set add_free gave, training on its own records (min_train_pairs 0): count ms, score ms
            (kg_coding_stats), wall ms, pairs and what was dropped; and the factor (count + score) / add_free device ms.
The first repetition of an input carries the module load or the first allocations of its size: leave it out and read the
median and the spread of the others (a device window here is 0.07 to 2 ms, so one repetition says little).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def _emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def _offsets(contigs):
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in contigs])
    return off


def stand_in_regions(seq, off, min_res: int = 300) -> np.ndarray:
    """The batch's free ORFs of min_res residues as regions of their own extent and frame."""
    orfs, _, _ = hotpath.free_orfs(seq, off, min_res)
    regs = np.zeros(len(orfs), dtype=N.REGION_DTYPE)
    for name in ("seq", "strand", "left", "right"):
        regs[name] = orfs[name]
    # (without the stop codon: a region that holds it would read as interrupted)
    stop = (orfs["flags"] & N.ORF_HAS_STOP) != 0
    regs["right"] -= np.where(stop & (orfs["strand"] == 0), 3, 0).astype(np.int32)
    regs["left"] += np.where(stop & (orfs["strand"] == 1), 3, 0).astype(np.int32)
    regs["fI"], regs["score"], regs["weighted"], regs["n_calls"], regs["kept"] = 0, 10, 1.0, 1, 1
    regs["best_frame"] = orfs["frame"]
    regs["frames"] = np.uint32(1) << orfs["frame"].astype(np.uint32)
    return regs


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coding_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    lib = N.load()
    genome = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))[1]
    total = sum(len(c) for c in genome)
    inputs = [("ecoli", genome, None), ("ecoli_x8", genome * 8, None), ("all_A", [b"A" * total], "one")]
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
        for rep in range(a.reps):
            ev, both, scored = C.c_void_p(), C.c_void_p(), C.c_void_p()
            N.check(lib.kg_orfs_regions(0, C.byref(N.KgOrfParams(7, 1, 0)), regs.ctypes.data, len(regs), seq.ctypes.data, off.ctypes.data,
                                        len(off) - 1, C.byref(ev)))
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                N.check(lib.kg_orfset_add_free(ev, C.byref(N.KgFreeParams(100, 7, 0)), *args, C.byref(both)))
                wall_free = (time.perf_counter() - t0) * 1e3
                try:
                    ost = N.KgOrfStats()
                    N.check(lib.kg_orfset_stats(both, C.byref(ost)))
                    t0 = time.perf_counter()
                    N.check(lib.kg_orfset_coding(both, C.byref(N.KgCodingParams(0, 0, 0)), None, *args, C.byref(scored)))
                    wall = (time.perf_counter() - t0) * 1e3
                    try:
                        st = N.KgCodingStats()
                        N.check(lib.kg_orfset_coding_stats(scored, C.byref(st)))
                    finally:
                        lib.kg_orfset_free(scored)
                finally:
                    lib.kg_orfset_free(both)
            finally:
                lib.kg_orfset_free(ev)
            _emit(a.out, dict(base, what="add_free", rep=rep, device_ms=round(ost.ms, 3), wall_ms=round(wall_free, 2), orfs=int(ost.orfs)))
            d = st.as_dict()
            _emit(a.out, dict(base, what="coding", rep=rep, wall_ms=round(wall, 2), count_ms=round(d.pop("ms_count"), 3),
                              score_ms=round(d.pop("ms_score"), 3), coding_over_add_free=round((st.ms_count + st.ms_score) / ost.ms, 3), **d))
    return 0


if __name__ == "__main__":
    sys.exit(main())
