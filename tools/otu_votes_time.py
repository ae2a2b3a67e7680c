"""Time of tallying the OTU votes of a scan on the GPU (kg_result_otu_votes), one JSON line per measurement.

    python tools/otu_votes_time.py [--proteins 2000000] [--length 100] [--reps 3] [--out profiles/otu_votes_time.jsonl] [--only NAME]

  ecoli_genome      kg_result_otu_votes on a DNA scan of the E. coli genome (tests/golden) against a table derived from its
                    proteome with random OTU labels (min_proteins 1, purity 1): a handful of contigs with many hits each
  config5           the same on BASELINE config 5 (100 Mbp assembled from signature k-mers)
  family_proteins   the same on an -a scan of --proteins family proteins (tests/signature_model.family_device; the table is
                    derived from the same proteins): millions of short tallies
  host_group        the host alternative on each of the three: the copy of the hit, event and CALL records to the host, and
                    the numpy model (tests/otu_votes_model.otu_votes) on them
Each line carries the library's device time, the call's wall time and the scan's ms_total of the same input.  Every device
result is checked against the numpy model.
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

import otu_votes_model as V  # noqa: E402
import signature_model as M  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def time_result(name, r, off, reps, out):
    per = r.stats["n_containers"] // max(r.stats["n_seqs"], 1)
    r.otu_votes(off)                              # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = r.otu_votes(off)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.vote_stats["ms"])
    t0 = time.perf_counter()
    rec = (r.hits(), r.container_hit_start(), r.hit_events(), r.calls(), r.container_call_start())
    t1 = time.perf_counter()
    want = V.otu_votes(*rec, len(off) - 1, per, off)
    t2 = time.perf_counter()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes(), name
    st = r.vote_stats
    emit(out, {"what": name, "seqs": int(len(off) - 1), "hits": st["hits"], "calls": int(r.stats["n_calls"]), "votes": st["votes"],
               "pairs": st["pairs"], "assigned": st["assigned"], "bins": st["bins"], "device_ms": round(min(dev), 4),
               "wall_ms": round(min(wall), 3), "scan_ms_total": round(r.stats["ms_total"], 3)})
    emit(out, {"what": "host_group", "of": name, "hits": st["hits"], "copy_ms": round((t1 - t0) * 1e3, 2),
               "numpy_model_ms": round((t2 - t1) * 1e3, 1)})


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


def family(n_prot, length, reps, out):
    seq, off, fn, otu = M.family_device(n_prot, length, 5, "cuda")
    with hotpath.derive_signatures(None, off, fn, otu, 2, 80, device_ptr=seq.data_ptr()) as s:
        tab = hotpath.SignatureTable.build(s.device_tensor(), default_num_sigs(s.count))
    torch.cuda.synchronize()
    with tab, tab.scan(None, off, hotpath.Params(aa=True), device_ptr=seq.data_ptr()) as r:
        time_result("family_proteins", r, off, reps, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["ecoli_genome", "config5", "family_proteins"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "otu_votes_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.only in (None, "ecoli_genome"):
            ecoli(a.reps, out)
        if a.only in (None, "config5"):
            config5(a.reps, out)
        if a.only in (None, "family_proteins"):
            family(a.proteins, a.length, a.reps, out)


if __name__ == "__main__":
    main()
