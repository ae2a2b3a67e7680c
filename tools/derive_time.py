"""Time of deriving signatures on the GPU (kg_signatures_derive*), one JSON line per measurement.

    python tools/derive_time.py [--proteins 3450000] [--length 320] [--reps 2] [--out profiles/derive_time.jsonl]

The training set is tests/signature_model.family_device: seeded protein families with point mutations, generated on the
device (about 10^9 windows at the defaults).
  device_derive  kg_signatures_derive_device, default pass size: wall ms and the library's own split (kg_derive_stats)
  host_derive    kg_signatures_derive from a pageable numpy array (upload through pinned pieces included)
  multi_pass     the device entry with max_windows_per_pass = valid windows / 6
  torch_model    tests/signature_model.derive (torch) on the same GPU
Every run's signatures are checked against the device entry's, and the device entry's against the model's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import signature_model as M  # noqa: E402
from kmergutsjava_amd import hotpath  # noqa: E402


def _emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=3_450_000)
    ap.add_argument("--length", type=int, default=320)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_time.jsonl"))
    ap.add_argument("--only-device", action="store_true", help="the device entry only (for a kernel trace)")
    a = ap.parse_args()
    seq, off, fn, otu = M.family_device(a.proteins, a.length, 901, "cuda")
    torch.cuda.synchronize()
    base = {"proteins": a.proteins, "windows": int((off[1:] - off[:-1] - 8).clip(0).sum()), "gpu": torch.cuda.get_device_name(0)}

    def run(what, **kw):
        ref = None
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with hotpath.derive_signatures(**kw) as s:
                wall = (time.perf_counter() - t0) * 1e3
                st = s.stats()
                got = s.numpy()
            if ref is None:
                ref = got
            assert got.tobytes() == ref.tobytes(), what
            _emit(a.out, dict(base, what=what, rep=rep, wall_ms=round(wall, 2), **{k: (round(v, 3) if isinstance(v, float) else v)
                                                                                    for k, v in st.items()}))
        return ref, st

    dev, st = run("device_derive", seq=None, offsets=off, fn=fn, otu=otu, device_ptr=seq.data_ptr())
    if a.only_device:
        return 0
    host_seq = seq.cpu().numpy()
    h, _ = run("host_derive", seq=host_seq, offsets=off, fn=fn, otu=otu)
    assert h.tobytes() == dev.tobytes()
    del host_seq, h
    m, _ = run("multi_pass", seq=None, offsets=off, fn=fn, otu=otu, device_ptr=seq.data_ptr(),
               max_windows_per_pass=st["valid_windows"] // 6 + 1)
    assert m.tobytes() == dev.tobytes()
    del m
    for rep in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = M.derive(seq, off, fn, otu)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert want.tobytes() == dev.tobytes()
        _emit(a.out, dict(base, what="torch_model", rep=rep, wall_ms=round(wall, 2), signatures=len(want)))
        del want
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
