"""Time of a table scan followed by the search of what it left unnamed (kg_result_search_residual) beside the plain translated
search of every fragment, on a genome whose table knows half of its proteins; one JSON line per measurement.

    python tools/residual_time.py [--reps 3] [--out profiles/residual_time.jsonl]

Input: the E. coli genome of tests/golden as the contigs.  The table holds the signatures of every second protein of its .faa
(proteins 0, 2, 4, ...; each protein its own function, named by its id, so min_proteins = 1 and the default purity: what
make_signatures -D writes for such an annotation); the index is built from the whole .faa.  The defaults of SearchDb.search_contigs
and ref = the fragment.  Repetitions 2 and 3 of --reps 3 are the ones to read: the first carries the contexts' start and is marked.
  residual    tab.scan, then SearchDb.search_contigs(explained_by=the result): wall ms, the scan's device time (ms_scan_total), the
              device times of kg_evidence_stats and of kg_residual_stats_of (ms_explain, ms_compact, ms_merge), their sum with the
              scan (ms_device), and the counts: explained and searched fragments and residues, CALLs of either kind
  plain       SearchDb.search_contigs without a table: wall ms and device times, the yardstick of the same run
  compact     the compaction's bytes (searched residues read and written, the records read and written) over ms_compact, beside
              a device-to-device hipMemcpyAsync of the searched residues' byte count, timed with events in this script
  regions     Evidence.regions of both ways: regions, kept ones, multi-frame ones, proteins that are the function of a kept region
"""
from __future__ import annotations

import argparse
import ctypes
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
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402

ALIGN = dict(ref="member")
ORF_BYTES = 48


def _golden(name: str):
    return parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name), "rb").read()))[1]


def _memcpy_ms(n_bytes: int, reps: int = 5) -> float:
    """The best of `reps` device-to-device hipMemcpyAsync calls of n_bytes on the null stream, between two events."""
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    src = torch.zeros(max(n_bytes, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    best = float("inf")
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.default_stream())
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n_bytes, 3, None)       # 3: hipMemcpyDeviceToDevice
        e1.record(torch.cuda.default_stream())
        torch.cuda.synchronize()
        assert rc == 0
        best = min(best, e0.elapsed_time(e1))
    return best


def _round(st):
    return {k: (round(v, 3) if k.startswith("ms_") else v) for k, v in st.items()}


def _regions(ev, goff):
    regs, _ = ev.regions(goff)
    kept = regs[regs["kept"] != 0]
    return dict(calls=len(ev.calls), regions=len(regs), kept=len(kept), multi_frame=int(ev.region_stats["multi_frame"]),
                functions_with_a_kept_region=int(np.unique(kept["fI"]).size))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    ecoli = [bytes(p) for p in _golden("Ecoli_K12_W3110.faa.gz")]
    contigs = [bytes(c) for c in _golden("Ecoli_K12_W3110.fna.gz")]
    known = ecoli[0::2]
    tseq, toff = M.pack(ecoli)
    kseq, koff = M.pack(known)
    gseq, goff = M.pack(contigs)
    garr = np.frombuffer(gseq, dtype=np.uint8)
    # one function index space: protein 2f is function f of the table, protein 2f + 1 gets an index behind the table's
    target_fn = np.array([d // 2 if d % 2 == 0 else len(known) + d // 2 for d in range(len(ecoli))], dtype=np.int32)
    base = {"input": "ecoli_genome_table_of_every_second_protein", "targets": len(ecoli), "table_proteins": len(known), "contigs": len(contigs),
            "nucleotides": int(goff[-1]), "gpu": gpu}
    with hotpath.derive_signatures(kseq, koff, np.arange(len(known), dtype=np.int32), np.zeros(len(known), dtype=np.int32), min_proteins=1) as sigs:
        base["signatures"] = sigs.count
        with hotpath.SignatureTable.build(sigs.device_tensor(), default_num_sigs(sigs.count)) as tab, \
                hotpath.SearchDb.build(np.frombuffer(tseq, dtype=np.uint8), toff, query_room=2 * int(goff[-1])) as db:
            for rep in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with tab.scan(garr, goff, hotpath.Params(aa=False)) as r:
                    ev = db.search_contigs(garr, goff, align=ALIGN, target_fn=target_fn, explained_by=r)
                    ms_scan = r.stats["ms_total"]
                wall = (time.perf_counter() - t0) * 1e3
                rs = ev.residual_stats
                _emit(a.out, dict(base, what="residual", rep=rep, first_of_process=rep == 0, wall_ms=round(wall, 2), ms_scan_total=round(ms_scan, 3),
                                  ms_device=round(ms_scan + rs["ms_total"], 3), **_round(ev.stats),
                                  **{("residual_" + k if k == "ms_total" else k): v for k, v in _round(rs).items()}))
                t0 = time.perf_counter()
                plain = db.search_contigs(garr, goff, align=ALIGN, target_fn=target_fn)
                wall = (time.perf_counter() - t0) * 1e3
                _emit(a.out, dict(base, what="plain", rep=rep, wall_ms=round(wall, 2), **_round(plain.stats)))
                if rep == a.reps - 1:
                    moved = 2 * rs["searched_residues"] + 2 * ORF_BYTES * rs["searched"] + 8 * rs["searched"]
                    copy_ms = _memcpy_ms(rs["searched_residues"])
                    _emit(a.out, dict(base, what="compact", bytes_moved=moved, ms_compact=round(rs["ms_compact"], 4),
                                      compact_gb_per_s=round(moved / rs["ms_compact"] / 1e6, 1) if rs["ms_compact"] > 0 else None,
                                      memcpy_bytes=rs["searched_residues"], ms_memcpy=round(copy_ms, 4),
                                      memcpy_gb_per_s=round(2 * rs["searched_residues"] / copy_ms / 1e6, 1) if copy_ms > 0 else None))
                    _emit(a.out, dict(base, what="regions", way="residual", **_regions(ev, goff)))
                    _emit(a.out, dict(base, what="regions", way="plain", **_regions(plain, goff)))
                ev.close()
                plain.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
