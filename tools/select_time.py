"""Time of selecting a non-overlapping gene set among regions on the GPU (kg_regionset_select / kg_select_intervals), one JSON
line per measurement.

    python tools/select_time.py [--candidates 10000000] [--reps 3] [--out profiles/select_time.jsonl] [--only NAME]

  ecoli_genome      ScanResult.select on a DNA scan of the E. coli genome (tests/golden) against a table derived from its
                    proteome with random labels, as tools/regions_time.py does: the library's device time of the selection, its
                    rounds and pairs, the wall time of regions + selection, beside the regions call's device time (the yardstick)
  config5           the same on BASELINE config 5 (100 Mbp assembled from signature k-mers)
  select_intervals  kg_select_intervals on --candidates synthetic intervals over 1000 contigs: device time and wall, upload of
                    the list included
Every device result is compared with the model (tests/select_model.select_fast), whose time is recorded too.
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

import select_model as S  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def model_ms(iv, got):
    t0 = time.perf_counter()
    want = S.select_fast(iv)
    ms = (time.perf_counter() - t0) * 1e3
    assert got.tobytes() == want.tobytes()
    return round(ms, 1)


def time_result(name, r, off, reps, out):
    r.select(off)                                   # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        regs, start, sel = r.select(off)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.select_stats["ms"])
    st = r.select_stats
    emit(out, {"what": name, "contigs": int(len(off) - 1), "nucleotides": int(off[-1]), "candidates": st["candidates"],
               "eligible": st["eligible"], "selected": st["selected"], "overlapped": st["overlapped"], "pairs": st["pairs"],
               "conflicts": st["conflicts"], "rounds": st["rounds"], "device_ms": round(min(dev), 4),
               "wall_ms_regions_and_select": round(min(wall), 3), "regions_device_ms": round(r.region_stats["ms"], 4),
               "scan_ms_total": round(r.stats["ms_total"], 3), "model_ms": model_ms(S.of_records(regs), sel)})


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
    dna = np.frombuffer(b"".join(contigs), dtype=np.uint8)
    with tab, tab.scan(dna, off, hotpath.Params()) as r:
        time_result("ecoli_genome", r, off, reps, out)


def config5(reps, out):
    seq, off, rec = synth.high_density_device(1000, 4167, 20_000_003, 8_000_000, 501, True, torch.device("cuda", 0))
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_device_ptr(rec.data_ptr(), 20_000_003, 0, keepalive=rec) as tab:
        tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()).close()
        with tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()) as r:
            time_result("config5", r, off, reps, out)


def synthetic(n, reps, out):
    rng = np.random.default_rng(3)
    n_seqs, L = 1000, 30_000_000
    iv = np.zeros(n, dtype=N.INTERVAL_DTYPE)
    iv["seq"] = rng.integers(0, n_seqs, size=n)
    iv["left"] = rng.integers(0, L, size=n)
    iv["right"] = iv["left"] + rng.integers(90, 3000, size=n)
    iv["score"] = rng.integers(1, 200, size=n)
    iv["eligible"] = rng.random(n) < 0.9
    hotpath.select_intervals(iv[:1000], n_seqs)
    dev, wall = [], []
    for _ in range(reps):
        st = {}
        t0 = time.perf_counter()
        got = hotpath.select_intervals(iv, n_seqs, stats=st)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["ms"])
    emit(out, {"what": "select_intervals", "contigs": n_seqs, "candidates": n, "eligible": st["eligible"], "selected": st["selected"],
               "overlapped": st["overlapped"], "pairs": st["pairs"], "conflicts": st["conflicts"], "rounds": st["rounds"],
               "device_ms": round(min(dev), 3), "wall_ms": round(min(wall), 2), "upload_mb": round(iv.nbytes / 1e6, 1),
               "model_ms": model_ms(iv, got)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["ecoli_genome", "config5", "select_intervals"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.only in (None, "ecoli_genome"):
            ecoli(a.reps, out)
        if a.only in (None, "config5"):
            config5(a.reps, out)
        if a.only in (None, "select_intervals"):
            synthetic(a.candidates, a.reps, out)


if __name__ == "__main__":
    main()
