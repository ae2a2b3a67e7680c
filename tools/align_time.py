"""Time and effect of verifying family edges by local alignment (kg_proteins_cluster_aligned), one JSON line per measurement.

    python tools/align_time.py [--reps 3] [--residues 10000000] [--sample 200] [--out profiles/align_time.jsonl]

Inputs: those of tools/cluster_time.py (the E. coli proteome of tests/golden; eight mutated copies of it; the synthetic set).
Per input and repetition (rep 0 is the process's first call of its kind and is reported like the others: read it separately):
  aligned   hotpath.cluster_proteins(align={}) from a host array: wall ms, the aligned pairs, their cells, ms_align, cells per
            second, ms_total, the family counts -- beside ms_total and the counts of the same run without alignment
Once per input:
  member    the same with ref = "member": families, largest, cut, skipped
  largest   the largest family without alignment, and what its members' families are with it (ids or indices, lengths)
  split     eight copies only: proteins whose eight copies are not all in one family, without and with alignment, both refs
  model     tests/align_model.align_model on --sample of the aligned pairs, evenly spaced; its records must equal the device's
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

import align_model as A  # noqa: E402
import cluster_model as M  # noqa: E402
import signature_model as SM  # noqa: E402
from cluster_time import _emit, mutated_copies  # noqa: E402
from kmergutsjava_amd import _native as N, hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

COUNTS = ("links", "edges", "families", "families_multi", "largest")


def _r(st):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k not in ("edge_records", "align")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--residues", type=int, default=10_000_000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ids, ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    n_fam = a.residues // (8 * 300)
    inputs = [("ecoli", M.pack(ecoli), ids), ("ecoli_x8_mutated", M.pack(mutated_copies(ecoli, 8, 12, 5)), None),
              ("synthetic", SM.family_set(n_fam, 8, 300, 0.03, 77)[:2], None)]
    for name, (seq, off), names in inputs:
        n = off.size - 1
        arr = np.frombuffer(seq, dtype=np.uint8)
        lens = off[1:] - off[:-1]
        base = {"input": name, "proteins": n, "residues": int(off[-1]), "gpu": gpu}
        for rep in range(a.reps):
            torch.cuda.synchronize()
            plain, pst = hotpath.cluster_proteins(arr, off)
            t0 = time.perf_counter()
            rec, st = hotpath.cluster_proteins(arr, off, align={})
            wall = (time.perf_counter() - t0) * 1e3
            al = st["align"]
            _emit(a.out, dict(base, what="aligned", rep=rep, wall_ms=round(wall, 2), pairs=al["aligned"], cut=al["cut"], skipped=al["skipped"],
                              cells=al["cells"], ms_align=round(al["ms_align"], 3),
                              cells_per_s=round(al["cells"] / (al["ms_align"] * 1e-3)) if al["ms_align"] > 0 else None,
                              ms_total=round(st["ms_total"], 3), ms_total_without=round(pst["ms_total"], 3),
                              **{k: st[k] for k in COUNTS}, **{k + "_without": pst[k] for k in COUNTS}))
        mrec, mst = hotpath.cluster_proteins(arr, off, align=dict(ref="member"))
        _emit(a.out, dict(base, what="member", cut=mst["align"]["cut"], skipped=mst["align"]["skipped"], **{k: mst[k] for k in COUNTS}))
        # the largest family without alignment, and where its members are with it
        root = int(np.bincount(plain["root"]).argmax())
        who = np.flatnonzero(plain["root"] == root)
        label = (lambda i: names[i].decode("latin-1")) if names is not None else (lambda i: int(i))
        _emit(a.out, dict(base, what="largest", size=int(who.size), members=[[label(i), int(lens[i])] for i in who[:64]],
                          families_with_alignment=sorted(np.bincount(np.unique(rec["root"][who], return_inverse=True)[1]).tolist(), reverse=True),
                          families_with_ref_member=sorted(np.bincount(np.unique(mrec["root"][who], return_inverse=True)[1]).tolist(), reverse=True),
                          largest_with_alignment=[[label(i), int(lens[i])] for i in
                                                  np.flatnonzero(rec["root"] == int(np.bincount(rec["root"]).argmax()))[:64]]))
        if name == "ecoli_x8_mutated":
            per = n // 8

            def split(r):
                roots = r["root"].reshape(8, per)
                return int((roots != roots[0]).any(axis=0).sum())

            _emit(a.out, dict(base, what="split", originals=per, split_without=split(plain), split_with_alignment=split(rec),
                              split_with_ref_member=split(mrec)))
        # the model on a sample of the aligned pairs
        e = st["edge_records"]
        done = np.flatnonzero(e["status"] != N.EDGE_SKIPPED)
        pick = done[np.linspace(0, done.size - 1, min(a.sample, done.size)).astype(np.int64)] if done.size else done
        t0 = time.perf_counter()
        want = A.align_model(seq, off, np.stack([e["member"][pick], e["centre"][pick]], axis=1))
        wall = (time.perf_counter() - t0) * 1e3
        assert (want["score"] == e["score"][pick]).all() and (want["end_a"] == e["end_member"][pick]).all() and \
            (want["end_b"] == e["end_centre"][pick]).all(), name
        cells = int((lens[e["member"][pick]] * lens[e["centre"][pick]]).sum())
        _emit(a.out, dict(base, what="model", sample=int(pick.size), sample_cells=cells, wall_ms=round(wall, 2),
                          cells_per_s=round(cells / (wall * 1e-3)) if wall > 0 else None))
    return 0


if __name__ == "__main__":
    sys.exit(main())
