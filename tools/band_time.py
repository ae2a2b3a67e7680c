"""Time and recall of the protein search with every candidate aligned in a band around its best seed diagonal
(kg_proteins_search_banded) beside the call it leaves in place, one JSON line per measurement.

    python tools/band_time.py [--reps 3] [--residues 10000000] [--out profiles/band_time.jsonl]

Inputs: those of tools/ungapped_search_time.py (the E. coli proteome of tests/golden against one mutated copy of it, a
substitution at about every 12th residue; a synthetic set of --residues residues split in two), and the proteome against a copy
whose every protein also carries an insertion or a deletion of 1 to 10 residues about every 50th residue: without indels a band
loses nothing by construction.  The first repetition of the process is marked and left out of the means.  Seeds: `reduced`.
Per input, repetition and setting (`off`: kg_proteins_search_filtered at min_score 0, the yardstick, in the same run; W of 8,
16, 32, 64 and 128):
  search    the library's device times, the aligned pairs, band cells against full cells, the queries with a rank-0 hit, those
            whose rank-0 hit is on a target with their original's sequence (proteome inputs), and the records whose banded score
            is below the yardstick's score for the same (query, target)
Per input and setting once, over the repetitions but the first:
  mean      the times, averaged
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

import band_model as B  # noqa: E402
import cluster_model as M  # noqa: E402
import signature_model as SM  # noqa: E402
from cluster_time import _emit, mutated_copies  # noqa: E402
from search_time import _rounded, originals_first  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

SETTINGS = (("off", None), ("W8", 8), ("W16", 16), ("W32", 32), ("W64", 64), ("W128", 128))
KEYS = ("ms_encode", "ms_sort", "ms_join", "ms_align", "ms_total")


def run(arr, off, n_db, band):
    hits, start, st, _ = hotpath.search_proteins(arr, off, n_db, seeds="reduced", ungapped=True, band=band)
    b = st.pop("band", dict(band_cells=st["cells"], full_cells=st["cells"]))
    st.pop("ungapped")
    return hits, start, dict(st, band_cells=b["band_cells"], full_cells=b["full_cells"])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    n_fam = a.residues // (8 * 300)
    sseq, soff = SM.family_set(n_fam, 8, 300, 0.03, 77)[:2]
    synth = [bytes(sseq[soff[k]:soff[k + 1]]) for k in range(len(soff) - 1)]
    mutated = mutated_copies(ecoli, 1, 12, 5)
    rng = np.random.default_rng(50)
    inputs = [("ecoli_vs_mutated", ecoli + mutated, len(ecoli), True),
              ("ecoli_vs_mutated_indels", ecoli + [B.with_indels(rng, bytes(p), 50, 10) for p in mutated], len(ecoli), True),
              ("synthetic_halves", synth[0::2] + synth[1::2], len(synth[0::2]), False)]
    first = True
    for name, prots, n_db, has_origin in inputs:
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        base = {"input": name, "targets": n_db, "queries": len(prots) - n_db, "residues": int(off[-1]), "gpu": gpu, "seeds": "reduced"}
        kept = {setting: [] for setting, _ in SETTINGS}
        full_score = None
        for rep in range(a.reps):
            for setting, band in SETTINGS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hits, start, st = run(arr, off, n_db, band)
                wall = (time.perf_counter() - t0) * 1e3
                key = hits["query"].astype(np.int64) * n_db + hits["target"]
                order = np.argsort(key, kind="stable")
                if band is None:
                    full_score = (key[order], hits["score"][order])
                below = -1
                if full_score is not None and np.array_equal(full_score[0], key[order]):
                    below = int((hits["score"][order] < full_score[1]).sum())
                more = {}
                if has_origin:
                    more["original_first"] = originals_first(prots, n_db, hits, start, list(range(n_db)))
                _emit(a.out, dict(base, what="search", setting=setting, rep=rep, first_of_process=first, wall_ms=round(wall, 2),
                                  records=len(hits), below_full=below, **more, **_rounded(st)))
                first = False
                if rep > 0:
                    kept[setting].append(st)
        for setting, sts in kept.items():
            if sts:
                _emit(a.out, dict(base, what="mean", setting=setting, reps_kept=len(sts), aligned=sts[0]["aligned"],
                                  band_cells=sts[0]["band_cells"], full_cells=sts[0]["full_cells"],
                                  **{k: round(float(np.mean([st[k] for st in sts])), 3) for k in KEYS}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
