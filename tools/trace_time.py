"""Time of the traceback pass behind a protein search on the GPU (kg_proteins_search_paths), one JSON line per measurement.

    python tools/trace_time.py [--reps 3] [--residues 10000000] [--out profiles/trace_time.jsonl]

The two inputs of tools/search_time.py.  Per input and repetition (the first repetition of the process is marked: it carries
the context's start), all times from the library's own events:
  plain     hotpath.search_proteins without paths: ms_align and ms_total, the yardstick of the same run
  hits      ... with paths="hits": ms_trace, the traced records, their box cells, cells per second, ms_trace / the plain ms_align
            of the same repetition, and ms_align / ms_total of this call (they exclude ms_trace)
  all       ... with paths="all"
The hit records of the three calls are compared byte for byte.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_time.jsonl"))
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
            hits, start, st = hotpath.search_proteins(arr, off, n_db)
            wall = (time.perf_counter() - t0) * 1e3
            _emit(a.out, dict(base, what="plain", rep=rep, first_of_process=first, wall_ms=round(wall, 2), records=len(hits), aligned=st["aligned"],
                              hits=st["hits"], cells=st["cells"], ms_align=round(st["ms_align"], 3), ms_total=round(st["ms_total"], 3)))
            first = False
            for mode in ("hits", "all"):
                t0 = time.perf_counter()
                h2, s2, pth, pst = hotpath.search_proteins(arr, off, n_db, paths=mode)
                wall = (time.perf_counter() - t0) * 1e3
                assert h2.tobytes() == hits.tobytes() and s2.tobytes() == start.tobytes()
                traced = pth[pth["status"] == 0]
                _emit(a.out, dict(base, what=mode, rep=rep, wall_ms=round(wall, 2), ms_trace=round(pst["ms_trace"], 3), traced=pst["traced"],
                                  untraced=pst["untraced"], box_cells=pst["trace_cells"],
                                  cells_per_s=round(pst["trace_cells"] / (pst["ms_trace"] * 1e-3)) if pst["ms_trace"] > 0 else None,
                                  trace_over_plain_align=round(pst["ms_trace"] / st["ms_align"], 3) if st["ms_align"] > 0 else None,
                                  box_cells_over_aligned_cells=round(pst["trace_cells"] / st["cells"], 3) if st["cells"] else None,
                                  ms_align=round(pst["ms_align"], 3), ms_total=round(pst["ms_total"], 3),
                                  with_gaps=int((traced["gap_opens"] > 0).sum()),
                                  mean_identity_pct=round(float(np.mean(100.0 * traced["identical"] / np.maximum(1, _columns(h2, pth)))), 2) if len(traced) else None))
    return 0


def _columns(hits, pth):
    t = pth["status"] == 0
    return ((hits["end_query"] - pth["start_a"] + 1) + pth["gap_cols_a"])[t]


if __name__ == "__main__":
    sys.exit(main())
