"""Time of a search against a resident protein database (kg_searchdb) beside the one-batch call, one JSON line per measurement.

    python tools/searchdb_time.py [--reps 3] [--out profiles/searchdb_time.jsonl]

Input, as tools/search_time.py makes it: the E. coli proteome of tests/golden as the database and one mutated copy of it (a
substitution at about every 12th residue, seeded) as the queries; the query sets are all of the copy, every 10th, every 100th and
one protein of it.  Repetitions 2 and 3 of --reps 3 are the ones to read: the first carries the context's start and is marked.
  build     kg_searchdb_build from a host array: wall ms and the library's split by stage (kg_searchdb_info)
  save      kg_searchdb_save: wall ms and the file's bytes
  open      kg_searchdb_open with the section checksums verified and, KG_SEARCHDB_NO_VERIFY=1, without: wall ms
  resident  SearchDb.search of a query set: wall ms, kg_search_stats' device times and the probe's (ms_probe, ms_upload), and
            ms_front = ms_encode + ms_sort + ms_join, the time in front of the alignment (ms_join holds ms_probe)
  onebatch  the yardstick of the same run and the same query set: hotpath.search_proteins on "targets, then queries", the same
            fields (no probe)
The records of the two calls are compared, byte for byte, once per query set.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("KG_ENABLE_TEST_HOOKS", "1")      # KG_SEARCHDB_NO_VERIFY is read only with it

import numpy as np  # noqa: E402

import cluster_model as M  # noqa: E402
from cluster_time import _emit, mutated_copies  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402

TIMES = ("ms_encode", "ms_sort", "ms_join", "ms_align", "ms_total")


def _row(st, wall):
    row = {k: round(st[k], 3) for k in TIMES}
    probe = st.get("db", {}).get("ms_probe", 0.0)
    row.update(wall_ms=round(wall, 2), ms_front=round(st["ms_encode"] + st["ms_sort"] + st["ms_join"], 3),
               join_pairs=st["join_pairs"], candidates=st["candidates"], aligned=st["aligned"], hits=st["hits"])
    if "db" in st:
        row.update(ms_probe=round(probe, 3), ms_upload=round(st["db"]["ms_upload"], 3), query_kmers=st["db"]["query_kmers"],
                   found=st["db"]["found"])
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "searchdb_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))[1]
    ecoli = [bytes(p) for p in ecoli]
    copies = mutated_copies(ecoli, 1, 12, 5)
    tseq, toff = M.pack(ecoli)
    tarr = np.frombuffer(tseq, dtype=np.uint8)
    base = {"input": "ecoli_vs_mutated", "targets": len(ecoli), "target_residues": int(toff[-1]), "gpu": gpu}
    path = os.path.join(tempfile.mkdtemp(), "ecoli.kgsdb")
    first = True
    for rep in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db = hotpath.SearchDb.build(tarr, toff)
        wall = (time.perf_counter() - t0) * 1e3
        info = db.info()
        _emit(a.out, dict(base, what="build", rep=rep, first_of_process=first, wall_ms=round(wall, 2), pairs=info["pairs"], kmers=info["kmers"],
                          device_bytes=info["device_bytes"], **{k: round(info[k], 3) for k in ("ms_upload", "ms_encode", "ms_sort", "ms_index", "ms_total")}))
        first = False
        t0 = time.perf_counter()
        db.save(path)
        _emit(a.out, dict(base, what="save", rep=rep, wall_ms=round((time.perf_counter() - t0) * 1e3, 2), file_bytes=os.path.getsize(path)))
        db.close()
        for verify in (True, False):
            if verify:
                os.environ.pop("KG_SEARCHDB_NO_VERIFY", None)
            else:
                os.environ["KG_SEARCHDB_NO_VERIFY"] = "1"
            t0 = time.perf_counter()
            opened = hotpath.SearchDb.open(path)
            _emit(a.out, dict(base, what="open", rep=rep, checksums_verified=verify, wall_ms=round((time.perf_counter() - t0) * 1e3, 2)))
            opened.close()
        os.environ.pop("KG_SEARCHDB_NO_VERIFY", None)
    with hotpath.SearchDb.open(path) as db:
        for step in (1, 10, 100, len(copies)):
            queries = copies[::step]
            qseq, qoff = M.pack(queries)
            qarr = np.frombuffer(qseq, dtype=np.uint8)
            bseq, boff = M.pack(ecoli + queries)
            barr = np.frombuffer(bseq, dtype=np.uint8)
            here = dict(base, queries=len(queries), query_residues=int(qoff[-1]))
            for rep in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = db.search(qarr, qoff)
                wall = (time.perf_counter() - t0) * 1e3
                _emit(a.out, dict(here, what="resident", rep=rep, **_row(got[2], wall)))
                t0 = time.perf_counter()
                one = hotpath.search_proteins(barr, boff, len(ecoli))
                wall = (time.perf_counter() - t0) * 1e3
                _emit(a.out, dict(here, what="onebatch", rep=rep, **_row(one[2], wall)))
                assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
    os.remove(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
