"""Time of assigning functions on the GPU (kg_result_assign / kg_assign_calls), one JSON line per measurement.

    python tools/assign_time.py [--proteins 5000000] [--length 100] [--calls 10000000] [--reps 3] [--out profiles/assign_time.jsonl]

  ecoli_result_assign   kg_result_assign on an -a scan of the E. coli proteome (tests/golden) against a table derived from it
                        with random labels (min_proteins 1, purity 1: every k-mer of an annotated protein): the library's device time (*ms) and the call's wall time
  family_result_assign  the same on an -a batch of --proteins family proteins (tests/signature_model.family_device; the table
                        is derived from the same proteins)
  assign_calls          kg_assign_calls on --calls synthetic CALL records (about two per protein): wall time, upload included
  host_group            the host alternative on the family batch: copy the CALLs, starts and OTU records down and group them
                        in numpy (tests/assign_model.assign)
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

import assign_model as A  # noqa: E402
import signature_model as M  # noqa: E402
from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402
from kmergutsjava_amd.make_table import default_num_sigs  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def time_result(r, reps):
    r.assign()                                    # warm: the block cache holds the scratch afterwards
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = r.assign()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.assign_ms)
    return got, min(dev), min(wall)


def scan_and_assign(name, seq_dev, seq_host, off, fn, otu, reps, out, host_group=False, minp=2, pur=80):
    with hotpath.derive_signatures(seq_host, off, fn, otu, minp, pur, device_ptr=None if seq_host is not None else seq_dev.data_ptr()) as s:
        S = default_num_sigs(s.count)
        tab = hotpath.SignatureTable.build(s.device_tensor(), S)
    with tab:
        params = hotpath.Params(aa=True)
        if seq_host is not None:
            r = tab.scan(seq_host, off, params)
        else:
            torch.cuda.synchronize()
            r = tab.scan(None, off, params, device_ptr=seq_dev.data_ptr())
        with r:
            got, dev_ms, wall_ms = time_result(r, reps)
            t0 = time.perf_counter()
            calls, ccs, ot = r.calls(), r.container_call_start(), r.otu()
            t1 = time.perf_counter()
            want = A.assign(calls, ccs, ot)
            t2 = time.perf_counter()
            assert got.tobytes() == want.tobytes(), name
            emit(out, {"what": name, "proteins": int(len(off) - 1), "calls": int(r.stats["n_calls"]), "device_ms": round(dev_ms, 4),
                       "wall_ms": round(wall_ms, 3), "scan_ms_total": round(r.stats["ms_total"], 3)})
            if host_group:
                emit(out, {"what": "host_group", "proteins": int(len(off) - 1), "calls": int(r.stats["n_calls"]),
                           "copy_ms": round((t1 - t0) * 1e3, 1), "numpy_group_ms": round((t2 - t1) * 1e3, 1),
                           "wall_ms": round((t2 - t0) * 1e3, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=5_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--calls", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as out:
        # E. coli
        ids, seqs = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz"), "rb").read()))
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in seqs])
        rng = np.random.default_rng(77)
        fn = rng.integers(0, 300, size=len(seqs)).astype(np.int32)
        fn[rng.random(len(seqs)) < 0.2] = -1
        otu = rng.integers(0, 4, size=len(seqs)).astype(np.int32)
        scan_and_assign("ecoli_result_assign", None, b"".join(seqs), off, fn, otu, a.reps, out, minp=1, pur=1)
        # kg_assign_calls on synthetic CALL lists
        n_prot = a.calls // 2
        rng = np.random.default_rng(3)
        cnt = rng.poisson(2.0, size=n_prot)
        cs = np.zeros(n_prot + 1, np.int64)
        cs[1:] = np.cumsum(cnt)
        m = int(cs[-1])
        calls = np.zeros(m, N.CALL_DTYPE)
        calls["fI"] = rng.integers(0, 20000, size=m)
        calls["count"] = rng.integers(5, 40, size=m)
        calls["weightedHits"] = (rng.random(m) * 20).astype(np.float32)
        hotpath.assign_calls(calls[:1000], np.minimum(cs[:501], 1000))
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = hotpath.assign_calls(calls, cs)
            wall.append((time.perf_counter() - t0) * 1e3)
        assert got.tobytes() == A.assign(calls, cs).tobytes()
        emit(out, {"what": "assign_calls", "proteins": n_prot, "calls": m, "wall_ms": round(min(wall), 2),
                   "upload_mb": round(m * 24 / 1e6, 1)})
        # a batch of family proteins
        seq, off, fn, otu = M.family_device(a.proteins, a.length, 5, "cuda")
        scan_and_assign("family_result_assign", seq, None, off, fn, otu, a.reps, out, host_group=True)


if __name__ == "__main__":
    main()
