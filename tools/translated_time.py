"""Time of a translated search (kg_contigs_search_translated) beside the same work done by the calls it is made of, and what it
finds on a genome whose proteins are the database; one JSON line per measurement.

    python tools/translated_time.py [--reps 3] [--out profiles/translated_time.jsonl]

Input: the E. coli genome of tests/golden as the contigs and an index of its proteome (the .faa of tests/golden) as the database,
with the defaults of SearchDb.search_contigs and ref = the fragment.  Repetitions 2 and 3 of --reps 3 are the ones to read: the
first carries the contexts' start and is marked.
  translated  SearchDb.search_contigs: wall ms (the copies of every array to the host included) and the device times of
              kg_evidence_stats (ms_fragments, ms_search, ms_calls, ms_total), with the counts
  parts       the yardstick of the same run: hotpath.free_orfs(start_codons=0) to the host, then SearchDb.search(paths="hits") of
              its proteins from the host: wall ms, and the two calls' device times (ms_fragments, ms_search, their sum ms_total)
  regions     Evidence.regions with its defaults: the regions, the kept ones, the multi-frame ones, and how many of the proteins
              are the target of a kept region
The hit records and paths of the two ways are compared, byte for byte, once.
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
from cluster_time import _emit  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

ALIGN = dict(ref="member")


def _golden(name: str):
    return parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name), "rb").read()))[1]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translated_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = [bytes(p) for p in _golden("Ecoli_K12_W3110.faa.gz")]
    contigs = [bytes(c) for c in _golden("Ecoli_K12_W3110.fna.gz")]
    tseq, toff = M.pack(ecoli)
    gseq, goff = M.pack(contigs)
    garr = np.frombuffer(gseq, dtype=np.uint8)
    base = {"input": "ecoli_genome_vs_proteome", "targets": len(ecoli), "target_residues": int(toff[-1]), "contigs": len(contigs),
            "nucleotides": int(goff[-1]), "gpu": gpu}
    with hotpath.SearchDb.build(np.frombuffer(tseq, dtype=np.uint8), toff, query_room=2 * int(goff[-1])) as db:
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = db.search_contigs(garr, goff, align=ALIGN)
            wall = (time.perf_counter() - t0) * 1e3
            st = ev.stats
            _emit(a.out, dict(base, what="translated", rep=rep, first_of_process=rep == 0, wall_ms=round(wall, 2),
                              **{k: (round(v, 3) if k.startswith("ms_") else v) for k, v in st.items()}))
            t0 = time.perf_counter()
            fst = {}
            recs, pstart, res = hotpath.free_orfs(garr, goff, min_res=30, start_codons=0, stats=fst)
            got = db.search(res, pstart, paths="hits", align=ALIGN)
            wall = (time.perf_counter() - t0) * 1e3
            ms_search = got[3]["ms_total"] + got[3]["ms_trace"]
            _emit(a.out, dict(base, what="parts", rep=rep, wall_ms=round(wall, 2), ms_fragments=round(fst["ms"], 3), ms_search=round(ms_search, 3),
                              ms_total=round(fst["ms"] + ms_search, 3), fragments=len(recs), fragment_residues=len(res), records=len(got[0])))
            if rep == 0:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], ev.search[:3]))
            if rep == a.reps - 1:
                regs, _ = ev.regions(goff)
                kept = regs[regs["kept"] != 0]
                _emit(a.out, dict(base, what="regions", calls=int(st["calls"]), regions=len(regs), kept=len(kept),
                                  multi_frame=int(ev.region_stats["multi_frame"]), ms_regions=round(ev.region_stats["ms"], 3),
                                  proteins_with_a_kept_region=int(np.unique(kept["fI"]).size)))
            ev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
