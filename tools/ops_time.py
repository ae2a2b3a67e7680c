"""Time of the ops behind a traced protein search on the GPU (KG_TRACE_OPS / KG_TRACE_OPS_EQX), one JSON line per measurement.

    python tools/ops_time.py [--reps 3] [--residues 10000000] [--out profiles/ops_time.jsonl]

The two inputs of tools/search_time.py and tools/trace_time.py.  Per input and repetition (the first repetition of the process
is marked: it carries the context's start), all times from the library's own events:
  paths     hotpath.search_proteins with paths="hits": ms_trace of the plain traceback, the yardstick of the same repetition
  m         ... with ops="m": ms_trace (the recording walk, the prefix sum and the fill: it replaces the plain trace), ms_ops (the
            prefix sum and the fill alone), the op count, ms_trace / the plain ms_trace and ms_ops / the plain ms_align
  eqx       ... with ops="eqx"
The hit and path records of the three calls are compared byte for byte.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import cluster_model as M  # noqa: E402
import signature_model as SM  # noqa: E402
from cluster_time import _emit, mutated_copies  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ops_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    n_fam = a.residues // (8 * 300)
    sseq, soff = SM.family_set(n_fam, 8, 300, 0.03, 77)[:2]
    synth = [bytes(sseq[soff[k]:soff[k + 1]]) for k in range(len(soff) - 1)]
    inputs = [("ecoli_vs_mutated", ecoli + mutated_copies(ecoli, 1, 12, 5), len(ecoli)),
              ("synthetic_halves", synth[0::2] + synth[1::2], len(synth[0::2]))]
    first = True
    for name, prots, n_db in inputs:
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        base = {"input": name, "targets": n_db, "queries": len(prots) - n_db, "residues": int(off[-1]), "gpu": gpu}
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hits, start, pth, st = hotpath.search_proteins(arr, off, n_db, paths="hits")
            wall = (time.perf_counter() - t0) * 1e3
            _emit(a.out, dict(base, what="paths", rep=rep, first_of_process=first, wall_ms=round(wall, 2), records=len(hits), traced=st["traced"],
                              box_cells=st["trace_cells"], ms_align=round(st["ms_align"], 3), ms_trace=round(st["ms_trace"], 3)))
            first = False
            for mode in ("m", "eqx"):
                t0 = time.perf_counter()
                h2, s2, p2, ost, op_start, ops = hotpath.search_proteins(arr, off, n_db, paths="hits", ops=mode)
                wall = (time.perf_counter() - t0) * 1e3
                assert h2.tobytes() == hits.tobytes() and s2.tobytes() == start.tobytes() and p2.tobytes() == pth.tobytes()
                assert op_start[-1] == len(ops) == ost["ops"]
                _emit(a.out, dict(base, what=mode, rep=rep, wall_ms=round(wall, 2), traced=ost["traced"], ops=ost["ops"],
                                  ops_per_traced=round(ost["ops"] / max(ost["traced"], 1), 2), op_bytes=int(ops.nbytes + op_start.nbytes),
                                  ms_trace=round(ost["ms_trace"], 3), ms_ops=round(ost["ms_ops"], 3),
                                  trace_over_plain_trace=round(ost["ms_trace"] / st["ms_trace"], 3) if st["ms_trace"] > 0 else None,
                                  ops_over_plain_align=round(ost["ms_ops"] / st["ms_align"], 3) if st["ms_align"] > 0 else None,
                                  ms_align=round(ost["ms_align"], 3)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
