"""Time of extending function regions to open reading frames and extracting their proteins on the GPU (kg_regionset_orfs /
kg_orfs_regions), one JSON line per measurement.

    python tools/orfs_time.py [--regions 10000000] [--reps 3] [--out profiles/orfs_time.jsonl] [--only NAME]

  ecoli_genome      ScanResult.orfs on a DNA scan of the E. coli genome (tests/golden) against a table derived from its proteome
                    with random labels, as tools/regions_time.py does: the library's device time of the ORF call, the wall time
                    of regions + ORFs, beside the scan's and the regions call's device time
  config5           the same on BASELINE config 5 (100 Mbp assembled from signature k-mers)
  orfs_regions      kg_orfs_regions on --regions synthetic regions over 100 Mbp of random contigs: device time and wall, upload
                    of the regions and the bytes included
  host_model        the host alternative: the numpy model (tests/orfs_model.orfs) on the same list, or, for lists of more than
                    --model-sample regions, on an evenly spaced sample of them (the record says which)
Every device result is checked against the numpy model (on the sample where one is taken).
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

import orfs_model as O  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def check_and_time_model(name, regs, seq, off, got, sample, out):
    """The numpy model on regs (or on `sample` evenly spaced ones), compared with the device's records and proteins."""
    idx = np.arange(len(regs)) if len(regs) <= sample else np.linspace(0, len(regs) - 1, sample).astype(np.int64)
    t0 = time.perf_counter()
    want = O.orfs(regs[idx], seq, off, only_kept=False)
    ms = (time.perf_counter() - t0) * 1e3
    orfs, ps, res = got
    assert orfs[idx].tobytes() == want[0].tobytes(), name
    kept = np.flatnonzero(ps[idx + 1] > ps[idx])
    for k in kept[:: max(1, len(kept) // 2000)]:
        i = idx[k]
        assert bytes(res[ps[i]:ps[i + 1]]) == bytes(want[2][want[1][k]:want[1][k + 1]]), (name, int(i))
    emit(out, {"what": "host_model", "of": name, "regions": int(len(regs)), "model_on": int(len(idx)), "numpy_model_ms": round(ms, 1),
               "numpy_model_ms_scaled_to_all": round(ms * len(regs) / max(len(idx), 1), 1)})


def time_result(name, r, seq_host, off, ptr, reps, sample, out):
    args = dict(device_ptr=ptr) if ptr else {}
    r.orfs(seq_host, off, **args)                  # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        regs, start, orfs, ps, res = r.orfs(seq_host, off, **args)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.orf_stats["ms"])
    st = r.orf_stats
    emit(out, {"what": name, "contigs": int(len(off) - 1), "nucleotides": int(off[-1]), "regions": st["orfs"], "complete": st["complete"],
               "interrupted": st["interrupted"], "residues": st["residues"], "tiles": st["tiles"], "device_ms": round(min(dev), 4),
               "wall_ms_regions_and_orfs": round(min(wall), 3), "regions_device_ms": round(r.region_stats["ms"], 4),
               "scan_ms_total": round(r.stats["ms_total"], 3), "bytes_on_device": bool(ptr)})
    seq = seq_host if seq_host is not None else torch.as_tensor(hotpath._DevMem(ptr, int(off[-1]), "|u1", None), device="cuda").cpu().numpy()
    full = r.orfs(seq_host, off, only_kept=False, **args)
    check_and_time_model(name, full[0], seq, off, full[2:], sample, out)


def ecoli(reps, sample, out):
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
        time_result("ecoli_genome", r, dna, off, None, reps, sample, out)


def config5(reps, sample, out):
    seq, off, rec = synth.high_density_device(1000, 4167, 20_000_003, 8_000_000, 501, True, torch.device("cuda", 0))
    torch.cuda.synchronize()
    with hotpath.SignatureTable.from_device_ptr(rec.data_ptr(), 20_000_003, 0, keepalive=rec) as tab:
        tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()).close()
        with tab.scan(None, off, hotpath.Params(), device_ptr=seq.data_ptr()) as r:
            time_result("config5", r, None, off, seq.data_ptr(), reps, sample, out)


def synthetic(n_regions, reps, sample, out):
    rng = np.random.default_rng(3)
    n_seqs, L = 1000, 100_000
    off = np.arange(n_seqs + 1, dtype=np.int64) * L
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n_seqs * L).astype(np.uint8)
    regs = np.zeros(n_regions, dtype=N.REGION_DTYPE)
    regs["seq"] = np.sort(rng.integers(0, n_seqs, size=n_regions))
    regs["strand"] = rng.integers(0, 2, size=n_regions)
    f = rng.integers(0, 3, size=n_regions)
    nf = (L - f) // 3
    j0 = rng.integers(0, nf - 40)
    j1 = j0 + rng.integers(0, 40, size=n_regions)
    xa, xb = f + 3 * j0, f + 3 * j1 + 2
    regs["left"] = np.where(regs["strand"] == 0, xa, L - 1 - xb)
    regs["right"] = np.where(regs["strand"] == 0, xb, L - 1 - xa)
    regs["best_frame"], regs["frames"], regs["kept"], regs["score"] = f, 1 << f, 1, 5
    hotpath.orf_regions(regs[:1000], seq, off)
    dev, wall = [], []
    for _ in range(reps):
        st = {}
        t0 = time.perf_counter()
        got = hotpath.orf_regions(regs, seq, off, only_kept=False, stats=st)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["ms"])
    emit(out, {"what": "orfs_regions", "contigs": n_seqs, "nucleotides": n_seqs * L, "regions": n_regions, "complete": st["complete"],
               "interrupted": st["interrupted"], "residues": st["residues"], "tiles": st["tiles"], "device_ms": round(min(dev), 3),
               "wall_ms": round(min(wall), 2), "upload_mb": round((regs.nbytes + seq.nbytes) / 1e6, 1)})
    check_and_time_model("orfs_regions", regs, seq, off, got, sample, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-sample", type=int, default=100_000)
    ap.add_argument("--only", default=None, choices=["ecoli_genome", "config5", "orfs_regions"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orfs_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.only in (None, "ecoli_genome"):
            ecoli(a.reps, a.model_sample, out)
        if a.only in (None, "config5"):
            config5(a.reps, a.model_sample, out)
        if a.only in (None, "orfs_regions"):
            synthetic(a.regions, a.reps, a.model_sample, out)


if __name__ == "__main__":
    main()
