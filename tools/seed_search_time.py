"""Time and recall of the seeded protein search on the GPU (kg_proteins_search_seeded) beside the exact one, one JSON line per
measurement.

    python tools/seed_search_time.py [--reps 3] [--residues 10000000] [--out profiles/seed_search_time.jsonl]

Inputs: the two of tools/search_time.py (the E. coli proteome of tests/golden against one mutated copy of it, a substitution at
about every 12th residue; a synthetic set of --residues residues split in two).
Per input and repetition (the first repetition of the process is marked: it carries the context's start):
  search    hotpath.search_proteins under `exact` (seeds=None: kg_proteins_search, the yardstick, in the same run) and under
            `reduced`: wall ms and the library's own split (kg_search_stats: the five device times, valid_windows, join_pairs,
            candidates, aligned).  Under `reduced`, ms_encode is the new kernel's two launches (the count pass and the emit
            pass) and nothing else; encode_share is its share of ms_total.
Per input once, over the repetitions but the first:
  ratio     reduced over exact: ms_total, and each ms_* part
Recall (E. coli proteome only), per substitution rate (every 12th, 6th, 4th and 3rd residue on average, fixed seed) and seed set:
  recall    the queries with a rank-0 hit, those whose rank-0 hit is on a target with their original's sequence, and the
            join_pairs and ms_total the call cost
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
from search_time import _rounded, originals_first  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

SEEDS = (("exact", None), ("reduced", "reduced"))
PARTS = ("ms_encode", "ms_sort", "ms_join", "ms_align", "ms_total")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_search_time.jsonl"))
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
        kept = {label: [] for label, _ in SEEDS}
        for rep in range(a.reps):
            for label, seeds in SEEDS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hits, start, st = hotpath.search_proteins(arr, off, n_db, seeds=seeds)
                wall = (time.perf_counter() - t0) * 1e3
                _emit(a.out, dict(base, what="search", seeds=label, rep=rep, first_of_process=first, wall_ms=round(wall, 2), records=len(hits),
                                  encode_share=round(st["ms_encode"] / st["ms_total"], 3), **_rounded(st)))
                first = False
                if rep > 0:
                    kept[label].append(st)
        if kept["exact"]:
            mean = {label: {k: float(np.mean([st[k] for st in sts])) for k in PARTS} for label, sts in kept.items()}
            _emit(a.out, dict(base, what="ratio", reps_kept=len(kept["exact"]),
                              **{"reduced_over_exact_" + k: round(mean["reduced"][k] / mean["exact"][k], 3) for k in PARTS},
                              **{"exact_" + k: round(mean["exact"][k], 3) for k in PARTS}, **{"reduced_" + k: round(mean["reduced"][k], 3) for k in PARTS}))
    origin = list(range(len(ecoli)))
    for every in (12, 6, 4, 3):
        prots = ecoli + mutated_copies(ecoli, 1, every, 5)
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        for label, seeds in SEEDS:
            hits, start, st = hotpath.search_proteins(arr, off, len(ecoli), seeds=seeds)
            _emit(a.out, dict(what="recall", input="ecoli_vs_mutated", substitution_every=every, seeds=label, queries=len(ecoli),
                              queries_hit=st["queries_hit"], original_first=originals_first(prots, len(ecoli), hits, start, origin),
                              valid_windows=st["valid_windows"], join_pairs=st["join_pairs"], candidates=st["candidates"], aligned=st["aligned"],
                              ms_total=round(st["ms_total"], 3), gpu=gpu))
    return 0


if __name__ == "__main__":
    sys.exit(main())
