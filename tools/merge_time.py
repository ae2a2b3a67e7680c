"""Time of merging new signatures into a resident table (kg_table_merge_signatures_device), one JSON line per measurement.

    python tools/merge_time.py [--out profiles/merge_time.jsonl] [--reps 3] [--full] [--conflicts 0.3]

Per configuration (table slots at load 0.5, new signatures, --conflicts of them on k-mers the table holds): the merge call's wall
time and the library's own split (kg_merge_stats: extract, sort, resolve, total; HIP-event times), and the yardstick of the same
run: kg_table_build_device on the merged set U (wall, and the KG_DEBUG split: sort, placement, fill/scatter, table_finish).
Configurations: 10^8 slots plus 10^6 and 10^7 new signatures; with --full the 1 400 303 159-slot table plus 10^7.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["KG_DEBUG"] = "1"

import torch  # noqa: E402

from build_time import _captured, _parts, _signatures  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402


def run(S, n_new, conflicts, reps, emit):
    dev = torch.device("cuda", 0)
    keys = synth.random_keys(int(S * 0.5), 202, dev)
    base_sig = _signatures(keys, 205)
    tab, _ = _captured(lambda: hotpath.SignatureTable.build(base_sig.view(torch.uint8).reshape(-1), S))
    del base_sig
    n_hit = int(n_new * conflicts)
    g = torch.Generator(device=dev).manual_seed(11)
    hit = keys[torch.randperm(keys.numel(), device=dev, generator=g)[:n_hit]]
    fresh = synth.random_keys(n_new, 909, dev)
    fresh = fresh[~torch.isin(fresh, keys)][:n_new - n_hit]
    new_keys = torch.cat([hit, fresh])
    del keys, hit, fresh
    new_sig = _signatures(new_keys, 911).view(torch.uint8).reshape(-1)
    del new_keys
    torch.cuda.empty_cache()
    for policy in ("keep", "replace", "drop"):
        for r in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u, _ = _captured(lambda: tab.merge_signatures(new_sig, on_conflict=policy))
            wall = (time.perf_counter() - t0) * 1e3
            st = u.merge_stats()
            row = dict(what="merge", policy=policy, rep=r, num_sigs=S, wall_ms=round(wall, 2))
            row.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()})
            if policy == "keep":                        # the yardstick: the parent's build of the same U
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                built, err = _captured(lambda: hotpath.SignatureTable.build(u.device_tensor(), S))
                bwall = (time.perf_counter() - t0) * 1e3
                parts = _parts(err)
                row.update(build_wall_ms=round(bwall, 2), build_placed=built.placed, **{"build_" + k: v for k, v in parts.items()})
                device_build = sum(parts.get(k, 0.0) for k in ("sort_ms", "place_ms", "fill_scatter_ms", "finish_ms"))
                if device_build:
                    row["build_device_ms"] = round(device_build, 3)
                    row["merge_over_build"] = round(st["ms_total"] / device_build, 3)
                row["merge_wall_over_build_wall"] = round(wall / bwall, 3)
                built.close()
            u.close()
            emit(**row)
    tab.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_time.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--conflicts", type=float, default=0.3)
    ap.add_argument("--full", action="store_true", help="also the 1 400 303 159-slot table plus 10^7 new signatures")
    a = ap.parse_args()
    with open(a.out, "w") as f:
        def emit(**kw):
            line = json.dumps(kw)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        configs = [(100_000_007, 1_000_000), (100_000_007, 10_000_000)] + ([(1_400_303_159, 10_000_000)] if a.full else [])
        for S, n_new in configs:
            run(S, n_new, a.conflicts, a.reps, emit)


if __name__ == "__main__":
    main()
