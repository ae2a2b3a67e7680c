"""Time and effect of the low-complexity mask on the GPU (kg_proteins_mask, kg_proteins_search_masked), one JSON line per
measurement.

    python tools/mask_time.py [--reps 5] [--residues 10000000] [--out profiles/mask_time.jsonl]

Inputs: the two of tools/search_time.py (the E. coli proteome of tests/golden against one mutated copy of it, a substitution at
about every 12th residue; a synthetic set of --residues residues split in two).
  share     hotpath.mask_proteins on the golden proteome alone: masked residues, share, segments, proteins touched, ms_mask
  search    per input and repetition, hotpath.search_proteins unmasked and with mask=True, exact and `reduced` seeds: the
            library's own split (kg_search_stats) and, masked, the mask's ms_mask beside ms_encode and ms_total
  recall    the 192 substituted queries of tests/test_gpu_seeded_search.py against the golden proteome: queries_hit, candidates,
            join_pairs and kmers_masked with and without the mask, exact and `reduced` seeds
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
from search_time import _rounded  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

ALPHA = b"ACDEFGHIKLMNPQRSTVWY"


def _mask_part(st):
    m = st["mask"]
    return dict(ms_mask=round(m["ms_mask"], 3), mask_over_encode=round(m["ms_mask"] / st["ms_encode"], 3),
                mask_share_of_total=round(m["ms_mask"] / st["ms_total"], 3), masked_residues=m["masked_residues"], segments=m["segments"])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    n_fam = a.residues // (8 * 300)
    sseq, soff = SM.family_set(n_fam, 8, 300, 0.03, 77)[:2]
    synth = [bytes(sseq[soff[k]:soff[k + 1]]) for k in range(len(soff) - 1)]
    inputs = [("ecoli_vs_mutated", ecoli + mutated_copies(ecoli, 1, 12, 5), len(ecoli)),
              ("synthetic_halves", synth[0::2] + synth[1::2], len(synth[0::2]))]
    seq, off = M.pack(ecoli)
    for rep in range(3):
        flags, segs, start, st = hotpath.mask_proteins(np.frombuffer(seq, dtype=np.uint8), off)
        _emit(a.out, dict(what="share", input="ecoli", rep=rep, gpu=gpu, share_pct=round(100.0 * st["masked_residues"] / st["residues"], 2),
                          **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}))
    first = True
    for name, prots, n_db in inputs:
        seq, off = M.pack(prots)
        arr = np.frombuffer(seq, dtype=np.uint8)
        base = {"input": name, "targets": n_db, "queries": len(prots) - n_db, "residues": int(off[-1]), "gpu": gpu}
        for rep in range(a.reps):
            for seeds in (None, "reduced"):
                for mask in (None, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    more = {} if mask is None else {"mask": mask}
                    hits, start, st = hotpath.search_proteins(arr, off, n_db, seeds=seeds, **more)
                    wall = (time.perf_counter() - t0) * 1e3
                    extra = _mask_part(st) if mask else {}
                    st = {k: v for k, v in st.items() if k != "mask"}
                    _emit(a.out, dict(base, what="search", seeds=seeds or "exact", masked=bool(mask), rep=rep, first_of_process=first,
                                      wall_ms=round(wall, 2), records=len(hits), **_rounded(st), **extra))
                    first = False
    pick = [k for k in range(0, len(ecoli), len(ecoli) // 192) if len(ecoli[k]) >= 60][:192]
    qs = [bytes(ALPHA[(ALPHA.index(ch) + 3) % 20] if i % 12 == 6 and ch in ALPHA else ch for i, ch in enumerate(ecoli[k])) for k in pick]
    seq, off = M.pack(list(ecoli) + qs)
    arr = np.frombuffer(seq, dtype=np.uint8)
    for seeds in (None, "reduced"):
        for mask in (None, True):
            more = {} if mask is None else {"mask": mask}
            hits, start, st = hotpath.search_proteins(arr, off, len(ecoli), seeds=seeds, **more)
            own = sum(1 for q in range(len(qs)) if start[q + 1] > start[q] and ecoli[int(hits[start[q]]["target"])] == ecoli[pick[q]])
            _emit(a.out, dict(what="recall", input="ecoli_192_substituted", seeds=seeds or "exact", masked=bool(mask), queries=len(qs),
                              queries_hit=st["queries_hit"], rank0_on_own_sequence=own, candidates=st["candidates"],
                              join_pairs=st["join_pairs"], kmers_masked=st["kmers_masked"], valid_windows=st["valid_windows"],
                              aligned=st["aligned"], ms_total=round(st["ms_total"], 3), gpu=gpu))
    return 0


if __name__ == "__main__":
    sys.exit(main())
