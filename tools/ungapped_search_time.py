"""Time and recall of the protein search with the ungapped filter on the GPU (kg_proteins_search_filtered) beside the calls it
leaves in place, one JSON line per measurement.

    python tools/ungapped_search_time.py [--reps 3] [--residues 10000000] [--out profiles/ungapped_search_time.jsonl]

Inputs and repetitions: those of tools/seed_search_time.py (the E. coli proteome of tests/golden against one mutated copy of it, a
substitution at about every 12th residue; a synthetic set of --residues residues split in two; the first repetition of the
process is marked and left out of the means).
Per input, repetition and seed set (`exact`, `reduced`):
  search    hotpath.search_proteins without the filter (kg_proteins_search / kg_proteins_search_seeded: the yardsticks, in the
            same run) and with it at min_score 0, 20, 40 and 60: the library's device times, ms_ungapped, candidates, aligned
            pairs, alignment cells, the diagonal cells scored, the candidates dropped and cut
Per input and seed set once, over the repetitions but the first:
  mean      the same, averaged, per setting
Recall (E. coli proteome only), per substitution rate (every 12th, 6th, 4th and 3rd residue), seed set and setting:
  recall    the queries with a rank-0 hit, those whose rank-0 hit is on a target with their original's sequence, and the
            aligned pairs and ms_total the call cost
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
SETTINGS = (("off", None), ("min0", 0), ("min20", 20), ("min40", 40), ("min60", 60))
KEYS = ("ms_encode", "ms_sort", "ms_join", "ms_align", "ms_total", "ms_ungapped", "candidates", "aligned", "cells", "ungapped_cells",
        "dropped", "cut")


def run(arr, off, n_db, seeds, min_score):
    """-> (hits, hit_start, the statistics flattened: the ungapped ones beside the search's, 0 without the filter)"""
    if min_score is None:
        hits, start, st = hotpath.search_proteins(arr, off, n_db, seeds=seeds)
        u = dict(ms_ungapped=0.0, cells=0, dropped=0, cut=0)
    else:
        hits, start, st, _ = hotpath.search_proteins(arr, off, n_db, seeds=seeds, ungapped=dict(min_score=min_score))
        u = st.pop("ungapped")
    st = dict(st, ms_ungapped=u["ms_ungapped"], ungapped_cells=u["cells"], dropped=u["dropped"], cut=u["cut"])
    return hits, start, st


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ungapped_search_time.jsonl"))
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
        kept = {(label, setting): [] for label, _ in SEEDS for setting, _ in SETTINGS}
        for rep in range(a.reps):
            for label, seeds in SEEDS:
                for setting, min_score in SETTINGS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hits, start, st = run(arr, off, n_db, seeds, min_score)
                    wall = (time.perf_counter() - t0) * 1e3
                    _emit(a.out, dict(base, what="search", seeds=label, ungapped=setting, rep=rep, first_of_process=first,
                                      wall_ms=round(wall, 2), records=len(hits), **_rounded(st)))
                    first = False
                    if rep > 0:
                        kept[(label, setting)].append(st)
        for (label, setting), sts in kept.items():
            if sts:
                _emit(a.out, dict(base, what="mean", seeds=label, ungapped=setting, reps_kept=len(sts),
                                  **{k: round(float(np.mean([st[k] for st in sts])), 3) for k in KEYS}))
    origin = list(range(len(ecoli)))
    for every in (12, 6, 4, 3):
        prots = ecoli + mutated_copies(ecoli, 1, every, 5)
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        for label, seeds in SEEDS:
            for setting, min_score in SETTINGS:
                hits, start, st = run(arr, off, len(ecoli), seeds, min_score)
                _emit(a.out, dict(what="recall", input="ecoli_vs_mutated", substitution_every=every, seeds=label, ungapped=setting,
                                  queries=len(ecoli), queries_hit=st["queries_hit"],
                                  original_first=originals_first(prots, len(ecoli), hits, start, origin), candidates=st["candidates"],
                                  aligned=st["aligned"], dropped=st["dropped"], cut=st["cut"], ms_ungapped=round(st["ms_ungapped"], 3),
                                  ms_align=round(st["ms_align"], 3), ms_total=round(st["ms_total"], 3), gpu=gpu))
    return 0


if __name__ == "__main__":
    sys.exit(main())
