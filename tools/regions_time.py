"""Time of merging CALL records into function regions on the GPU (kg_result_regions / kg_regions_calls), one JSON line per
measurement.

    python tools/regions_time.py [--calls 10000000] [--reps 3] [--out profiles/regions_time.jsonl] [--only NAME]

  ecoli_genome      kg_result_regions on a DNA scan of the E. coli genome (tests/golden) against a table derived from its
                    proteome with random labels (min_proteins 1, purity 1): the library's device time and the call's wall time,
                    beside the scan's device time
  config5           the same on BASELINE config 5 (100 Mbp assembled from signature k-mers, about 3e5 CALLs)
  regions_calls     kg_regions_calls on --calls synthetic CALL records: device time and wall, upload included
  host_group        the host alternative on the same lists: the numpy model (tests/regions_model.regions); for the two scans
                    the copy of the CALL records to the host is timed as well
Every device result is checked against the numpy model.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import regions_model as R  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def time_result(name, r, off, reps, out):
    r.regions(off)                                # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = r.regions(off)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.region_stats["ms"])
    t0 = time.perf_counter()
    calls = r.calls()
    t1 = time.perf_counter()
    want = R.regions(calls, off)
    t2 = time.perf_counter()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), name
    st = r.region_stats
    emit(out, {"what": name, "contigs": int(len(off) - 1), "calls": st["calls"], "groups": st["groups"], "regions": st["regions"],
               "multi_frame": st["multi_frame"], "device_ms": round(min(dev), 4), "wall_ms": round(min(wall), 3),
               "scan_ms_total": round(r.stats["ms_total"], 3)})
    emit(out, {"what": "host_group", "of": name, "calls": st["calls"], "copy_ms": round((t1 - t0) * 1e3, 2),
               "numpy_group_ms": round((t2 - t1) * 1e3, 1)})


def ecoli(reps, out):
    gold = os.path.join(ROOT, "tests", "golden")
    _, seqs = parse_fasta(gzip.decompress(open(os.path.join(gold, "Ecoli_K12_W3110.faa.gz"), "rb").read()))
    poff = np.zeros(len(seqs) + 1, dtype=np.int64)
    poff[1:] = np.cumsum([len(x) for x in seqs])
    rng = np.random.default_rng(77)
    fn = rng.integers(0, 300, size=len(seqs)).astype(np.int32)
    fn[rng.random(len(seqs)) < 0.2] = -1
    otu = rng.integers(0, 4, size=len(seqs)).astype(np.int32)
    with hotpath.derive_signatures(b"".join(seqs), poff, fn, otu, 1, 1) as s:
        tab = hotpath.SignatureTable.build(s.device_tensor(), default_num_sigs(s.count))
    _, contigs = parse_fasta(gzip.decompress(open(os.path.join(gold, "Ecoli_K12_W3110.fna.gz"), "rb").read()))
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in contigs])
    with tab, tab.scan(b"".join(contigs), off, hotpath.Params()) as r:
        time_result("ecoli_genome", r, off, reps, out)


def config5(reps, out):
    seq, off, rec = synth.high_density_device(1000, 4167, 20_000_003, 8_000_000, 501, True, torch.device("cuda", 0))
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_device_ptr(rec.data_ptr(), 20_000_003, 0, keepalive=rec) as tab:
        tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()).close()
        with tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()) as r:
            time_result("config5", r, off, reps, out)


def synthetic(n_calls, reps, out):
    rng = np.random.default_rng(3)
    calls, off = R.random_calls_large(rng, max(1, n_calls // 300), n_calls, 20000, contig_len=100_000, span=120)
    hotpath.region_calls(calls[:1000], off)
    dev, wall = [], []
    for _ in range(reps):
        st = {}
        t0 = time.perf_counter()
        got = hotpath.region_calls(calls, off, stats=st)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["ms"])
    t0 = time.perf_counter()
    want = R.regions(calls, off)
    t1 = time.perf_counter()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    emit(out, {"what": "regions_calls", "contigs": int(len(off) - 1), "calls": int(len(calls)), "groups": st["groups"],
               "regions": st["regions"], "device_ms": round(min(dev), 3), "wall_ms": round(min(wall), 2),
               "upload_mb": round(len(calls) * 24 / 1e6, 1)})
    emit(out, {"what": "host_group", "of": "regions_calls", "calls": int(len(calls)), "numpy_group_ms": round((t1 - t0) * 1e3, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["ecoli_genome", "config5", "regions_calls"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.only in (None, "ecoli_genome"):
            ecoli(a.reps, out)
        if a.only in (None, "config5"):
            config5(a.reps, out)
        if a.only in (None, "regions_calls"):
            synthetic(a.calls, a.reps, out)


if __name__ == "__main__":
    main()
