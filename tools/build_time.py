"""Time of building signature tables on the GPU (kg_table_build*, kg_table_save), one JSON line per measurement.

    python tools/build_time.py [--num-sigs 1400303159] [--load 0.5] [--reps 2] [--save-dir DIR] [--no-save] [--no-host] [--no-dense]

  device_build   kg_table_build_device from shuffled device signatures: wall ms, and the library's own split (KG_DEBUG line:
                 sort, placement, fill/scatter, table_finish, HIP-event times)
  host_build     kg_table_build from a pageable numpy array (upload through pinned pieces included)
  synth_build    synth.build_table (torch) on the same GPU, same keys
  save_plain     kg_table_save to a plain file under --save-dir (default: a temporary directory, removed afterwards;
                 skipped when the file system has no room)
  dense_finish   a 10^8-slot table at load 0.9 built on the device: table_finish's part on a dense table
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["KG_DEBUG"] = "1"

import torch  # noqa: E402

from kmergutsjava_amd import hotpath, synth  # noqa: E402


def _signatures(keys, seed):
    otu, avg, fn, wt = synth.payload_of(keys, seed)
    sig = torch.stack([(keys & 0xFFFFFFFF).to(torch.int32), (keys >> 32).to(torch.int32), otu, avg, fn,
                       wt.contiguous().view(torch.int32)], dim=1)
    perm = torch.randperm(keys.numel(), device=keys.device, generator=torch.Generator(device=keys.device).manual_seed(7))
    return sig[perm].contiguous()


def _captured(fn):
    """run fn() with fd 2 sent to a file; returns (fn's value, the text written there)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode("utf-8", "replace")


def _parts(text):
    m = re.search(r"kg_table_build: .*sort_ms=([\d.]+) place_ms=([\d.]+) fill_scatter_ms=([\d.]+) finish_ms=([\d.]+)", text)
    return dict(zip(("sort_ms", "place_ms", "fill_scatter_ms", "finish_ms"), map(float, m.groups()))) if m else {}


def _timed_build(src, num_sigs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tab, err = _captured(lambda: hotpath.SignatureTable.build(src, num_sigs))
    ms = (time.perf_counter() - t0) * 1e3
    return tab, ms, _parts(err)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-sigs", type=int, default=1_400_303_159)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-save", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    S = a.num_sigs
    keys = synth.random_keys(int(S * a.load), 202, dev)
    n = keys.numel()
    pay = synth.payload_of(keys, 205)
    for r in range(a.reps):                                  # the torch formulation (records only)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec, placed = synth.build_table(keys, pay, S)
        torch.cuda.synchronize()
        emit(what="synth_build", rep=r, n=n, num_sigs=S, placed=placed, ms=round((time.perf_counter() - t0) * 1e3, 2))
        if r + 1 < a.reps:
            del rec
            torch.cuda.empty_cache()
    sig = _signatures(keys, 205)
    del keys, pay
    torch.cuda.empty_cache()
    flat = sig.view(torch.uint8).reshape(-1)
    for r in range(a.reps):
        tab, ms, parts = _timed_build(flat, S)
        same = torch.equal(tab.device_entries(), rec.view(torch.uint8).reshape(-1))
        emit(what="device_build", rep=r, n=n, num_sigs=S, placed=tab.placed, equal_to_synth=same, ms=round(ms, 2), **parts)
        if r + 1 < a.reps:
            tab.close()
    del rec
    torch.cuda.empty_cache()
    d = a.save_dir or tempfile.mkdtemp(prefix="kg_build_time_")
    need = 24 + S * 24
    try:
        if a.no_save:
            pass
        elif shutil.disk_usage(d).free > need + (4 << 30):
            p = os.path.join(d, "kmer.table.mem_map")
            t0 = time.perf_counter()
            tab.save(p)
            ms = (time.perf_counter() - t0) * 1e3
            emit(what="save_plain", bytes=os.path.getsize(p), ms=round(ms, 2), gb_per_s=round(need / ms / 1e6, 2))
            os.unlink(p)
        else:
            emit(what="save_plain", skipped="not enough free space in %s for %d bytes" % (d, need))
    finally:
        if not a.save_dir:
            shutil.rmtree(d, ignore_errors=True)
    tab.close()
    if not a.no_host:
        host = sig.cpu().numpy().reshape(-1).view(hotpath.N.SIGNATURE_DTYPE)    # pageable
        del sig, flat
        torch.cuda.empty_cache()
        for r in range(a.reps):
            tab, ms, parts = _timed_build(host, S)
            emit(what="host_build", rep=r, n=n, num_sigs=S, placed=tab.placed, ms=round(ms, 2), **parts)
            tab.close()
        del host
    else:
        del sig, flat
    torch.cuda.empty_cache()
    if not a.no_dense:
        S2 = 100_000_007
        keys = synth.random_keys(int(S2 * 0.9), 303, dev)
        sig2 = _signatures(keys, 306)
        n2 = keys.numel()
        del keys
        for r in range(a.reps):
            tab, ms, parts = _timed_build(sig2.view(torch.uint8).reshape(-1), S2)
            emit(what="dense_finish", rep=r, n=n2, num_sigs=S2, placed=tab.placed, ms=round(ms, 2), **parts)
            tab.close()


if __name__ == "__main__":
    main()
