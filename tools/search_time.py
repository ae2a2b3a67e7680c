"""Time of searching proteins against a database on the GPU (kg_proteins_search), one JSON line per measurement.

    python tools/search_time.py [--reps 3] [--residues 10000000] [--out profiles/search_time.jsonl]

Inputs, as tools/cluster_time.py makes them: the E. coli proteome of tests/golden as the database against one mutated copy of it
as the queries (a substitution at about every 12th residue, seeded); a synthetic set of --residues residues
(tests/signature_model.family_set: seeded families of eight) split in two: the proteins of even index are the database, those of
odd index the queries, so that every family has four members on each side.
Per input and repetition (the first repetition of the process is marked: it carries the context's start):
  search    hotpath.search_proteins from a host array: wall ms and the library's own split (kg_search_stats: the five device
            times, join_pairs, candidates, aligned, cells)
  cluster   the yardstick of the same run: kg_proteins_cluster_aligned on the concatenated input, its ms_total
Per input once:
  finding   of the mutated queries, how many have a protein with their original's sequence as the rank-0 hit, under the
            defaults and under min_shared = 1 (E. coli input only: the synthetic queries have no single original)
"""
from __future__ import annotations

import argparse
import gzip
import json
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
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def _rounded(st):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}


def originals_first(seqs, n_db, hits, hit_start, origin):
    """Queries whose rank-0 record is a hit on a target with the sequence of the query's original."""
    n = 0
    for q in range(len(hit_start) - 1):
        if hit_start[q + 1] > hit_start[q]:
            h = hits[int(hit_start[q])]
            n += int(h["status"]) == N.SEARCH_HIT and seqs[int(h["target"])] == seqs[origin[q]]
    return n


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    n_fam = a.residues // (8 * 300)
    sseq, soff = SM.family_set(n_fam, 8, 300, 0.03, 77)[:2]
    synth = [bytes(sseq[soff[k]:soff[k + 1]]) for k in range(len(soff) - 1)]
    inputs = [("ecoli_vs_mutated", ecoli + mutated_copies(ecoli, 1, 12, 5), len(ecoli), list(range(len(ecoli)))),
              ("synthetic_halves", synth[0::2] + synth[1::2], len(synth[0::2]), None)]
    first = True
    for name, prots, n_db, origin in inputs:
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        base = {"input": name, "targets": n_db, "queries": len(prots) - n_db, "residues": int(off[-1]), "gpu": gpu}
        got = None
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hits, start, st = hotpath.search_proteins(arr, off, n_db)
            wall = (time.perf_counter() - t0) * 1e3
            assert got is None or got.tobytes() == hits.tobytes()
            got = hits
            _emit(a.out, dict(base, what="search", rep=rep, first_of_process=first, wall_ms=round(wall, 2), records=len(hits), **_rounded(st)))
            first = False
            t0 = time.perf_counter()
            _, cst = hotpath.cluster_proteins(arr, off, align={})
            wall = (time.perf_counter() - t0) * 1e3
            _emit(a.out, dict(base, what="cluster", rep=rep, wall_ms=round(wall, 2), search_over_cluster_device=round(st["ms_total"] / cst["ms_total"], 3),
                              ms_total=round(cst["ms_total"], 3), ms_align=round(cst["align"]["ms_align"], 3), aligned=cst["align"]["aligned"],
                              cells=cst["align"]["cells"]))
        if origin is not None:
            h1, s1, st1 = hotpath.search_proteins(arr, off, n_db, min_shared=1)
            _emit(a.out, dict(base, what="finding", original_first_defaults=originals_first(prots, n_db, got, start, origin),
                              queries_hit_defaults=st["queries_hit"], original_first_min_shared_1=originals_first(prots, n_db, h1, s1, origin),
                              queries_hit_min_shared_1=st1["queries_hit"], candidates_min_shared_1=st1["candidates"],
                              join_pairs=st1["join_pairs"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
