"""Time of enumerating the evidence-free open reading frames of a batch on the GPU (kg_orfs_free / kg_orfset_add_free), one JSON
line per measurement.

    python tools/free_orfs_time.py [--mbp 100] [--reps 3] [--out profiles/free_orfs_time.jsonl] [--only NAME]

  ecoli_genome   the E. coli genome (tests/golden) behind a DNA scan against a table derived from its proteome with random
                 labels, as tools/select_time.py does
  config5        BASELINE config 5's contigs (100 Mbp assembled from signature k-mers)
  synthetic      --mbp million random nucleotides in 1000 contigs, scanned against config 5's table
Every row holds the device time of kg_orfset_add_free from the library's events (the enumerator plus the copy of the parent's
records), the wall time of regions + ORFs + free ORFs, the candidate and residue counts, the model's time
(tests/free_orfs_model.free_orfs, whose bytes the device's must equal; skipped above --model-limit nucleotides), and two
yardsticks measured in the same run: the device time of kg_regionset_orfs on the same batch (the same summary pass plus a
per-region kernel), and the time to stream the batch's bytes twice at the streaming HBM rate DESIGN.md section 6 records
(6.29 TB/s).
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

import free_orfs_model as F  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402

HBM_STREAM_TBS = 6.29


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def time_result(name, r, dna, off, ptr, reps, model_limit, out):
    kw = dict(device_ptr=ptr) if ptr else {}
    seq = None if ptr else dna
    r.orfs(seq, off, free_min_res=100, **kw)             # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        regs, start, orfs, ps, res = r.orfs(seq, off, free_min_res=100, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.orf_stats["ms"])
    st = dict(r.orf_stats)
    r.orfs(seq, off, **kw)
    rec = {"what": name, "contigs": int(len(off) - 1), "nucleotides": int(off[-1]), "regions": int(len(regs)),
           "free_candidates": int(len(orfs) - len(regs)), "residues": int(st["residues"]), "device_ms": round(min(dev), 4),
           "wall_ms_regions_orfs_and_free": round(min(wall), 3), "regionset_orfs_device_ms": round(r.orf_stats["ms"], 4),
           "two_passes_at_hbm_rate_ms": round(2 * int(off[-1]) / (HBM_STREAM_TBS * 1e12) * 1e3, 4)}
    if dna is not None and int(off[-1]) <= model_limit:
        t0 = time.perf_counter()
        want = F.free_orfs(dna, off)
        rec["model_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        n = len(regs)
        assert orfs[n:].tobytes() == want[0].tobytes() and res[ps[n]:].tobytes() == want[2].tobytes()
    emit(out, rec)


def ecoli(reps, model_limit, out):
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
        time_result("ecoli_genome", r, dna, off, None, reps, model_limit, out)


def config5(reps, mbp, model_limit, out):
    seq, off, rec = synth.high_density_device(1000, 4167, 20_000_003, 8_000_000, 501, True, torch.device("cuda", 0))
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_device_ptr(rec.data_ptr(), 20_000_003, 0, keepalive=rec) as tab:
        if mbp is None:
            with tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()) as r:
                time_result("config5", r, seq.cpu().numpy(), off, seq.data_ptr(), reps, model_limit, out)
            return
        n = mbp * 1_000_000
        rnd = torch.from_numpy(np.frombuffer(b"ACGT", dtype=np.uint8).copy()).cuda()[torch.randint(0, 4, (n,), device="cuda")]
        roff = np.linspace(0, n, 1001).astype(np.int64)
        torch.cuda.synchronize()
        with tab.scan(None, roff, hotpath.Params(), device_ptr=rnd.data_ptr()) as r:
            time_result("synthetic", r, rnd.cpu().numpy(), roff, rnd.data_ptr(), reps, model_limit, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-limit", type=int, default=10_000_000, help="nucleotides up to which the model runs beside the device")
    ap.add_argument("--only", default=None, choices=["ecoli_genome", "config5", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_orfs_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.only in (None, "ecoli_genome"):
            ecoli(a.reps, a.model_limit, out)
        if a.only in (None, "config5"):
            config5(a.reps, None, a.model_limit, out)
        if a.only in (None, "synthetic"):
            config5(a.reps, a.mbp, a.model_limit, out)


if __name__ == "__main__":
    main()
