"""Time of clustering proteins into families on the GPU (kg_proteins_cluster), one JSON line per measurement.

    python tools/cluster_time.py [--reps 3] [--residues 10000000] [--out profiles/cluster_time.jsonl]

Inputs: the E. coli proteome of tests/golden; eight mutated copies of it, concatenated (a substitution at about every 12th
residue, seeded); a synthetic set of --residues residues (tests/signature_model.family_set: seeded families of eight).
Per input and repetition:
  cluster   hotpath.cluster_proteins from a host array: wall ms, the library's own split (kg_cluster_stats: pairs, links,
            edges, rounds, ms_*), and whether rounds exceeds 2 * log2(n_prot) + 4
  derive    the yardstick of the same run: kg_signatures_derive on the same proteins, every protein given fn 0
  model     tests/cluster_model.cluster_numpy on the CPU, once; its records must equal the device's
"""
from __future__ import annotations

import argparse
import gzip
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cluster_model as M  # noqa: E402
import signature_model as SM  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def _emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def mutated_copies(seqs, copies: int, every: int, seed: int):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(M.ALPHA, dtype=np.uint8)
    out = []
    for _ in range(copies):
        for s in seqs:
            a = np.frombuffer(s, dtype=np.uint8).copy()
            hit = rng.random(a.size) < 1.0 / every
            a[hit] = alpha[rng.integers(0, 20, size=int(hit.sum()))]
            out.append(a.tobytes())
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    n_fam = a.residues // (8 * 300)
    inputs = [("ecoli", M.pack(ecoli)), ("ecoli_x8_mutated", M.pack(mutated_copies(ecoli, 8, 12, 5))),
              ("synthetic", SM.family_set(n_fam, 8, 300, 0.03, 77)[:2])]
    for name, (seq, off) in inputs:
        n = off.size - 1
        arr = np.frombuffer(seq, dtype=np.uint8)
        base = {"input": name, "proteins": n, "residues": int(off[-1]), "gpu": gpu}
        fn, otu = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        got = None
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec, st = hotpath.cluster_proteins(arr, off)
            wall = (time.perf_counter() - t0) * 1e3
            assert got is None or got.tobytes() == rec.tobytes()
            got = rec
            _emit(a.out, dict(base, what="cluster", rep=rep, wall_ms=round(wall, 2), rounds_bound=round(2 * math.log2(max(n, 2)) + 4, 1),
                              rounds_over_bound=bool(st["rounds"] > 2 * math.log2(max(n, 2)) + 4),
                              **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}))
            t0 = time.perf_counter()
            with hotpath.derive_signatures(arr, off, fn, otu) as s:
                wall = (time.perf_counter() - t0) * 1e3
                ds = s.stats()
            _emit(a.out, dict(base, what="derive", rep=rep, wall_ms=round(wall, 2), cluster_over_derive_device=round(st["ms_total"] / ds["ms_total"], 3),
                              **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in ds.items()}))
        t0 = time.perf_counter()
        want, _ = M.cluster_numpy(seq, off)
        wall = (time.perf_counter() - t0) * 1e3
        assert want.tobytes() == got.tobytes(), name
        _emit(a.out, dict(base, what="model", wall_ms=round(wall, 2)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
