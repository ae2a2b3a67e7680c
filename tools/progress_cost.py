#!/usr/bin/env python3
"""What the lookup's info lines cost at BASELINE config 3 (1 Gbp contig mix, 33.6 GB table; bench.py's inputs): three scans,
alternated after warm-up -- plain, KG_F_PROGRESS (byte home index: the index pass summarises the misses' walks) and
KG_F_COUNTERS | KG_F_PROGRESS (the tags, the counting kernels: the only progress scan before).  Prints one JSON object:
per kind the per-rep ms_total / ms_scan and their medians."""
import json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmergutsjava_amd import hotpath as hp, synth

reps = int(os.environ.get("PC_REPS", "7"))
dev = torch.device("cuda", 0)
num_sigs = 1_400_303_159
rec, placed, keys = synth.random_table(num_sigs, 0.5, 202, dev)
del keys
off = synth.offsets_of(synth.contig_mix_lengths(1_000_000_000, 301))
seq = synth.random_dna(int(off[-1]), 302, dev)
torch.cuda.synchronize()
kinds = {"plain": hp.Params(), "progress": hp.Params(progress=True), "counters_progress": hp.Params(counters=True, progress=True)}
out = {k: {"ms_total": [], "ms_scan": []} for k in kinds}
with hp.SignatureTable.from_device_ptr(rec.data_ptr(), num_sigs, 0, keepalive=rec) as tab:
    for rep in range(reps + 1):
        for k, p in kinds.items():
            with tab.scan(None, off, p, device_ptr=seq.data_ptr()) as r:
                st = r.stats
                if rep == 0:                                   # warm-up
                    out[k]["part_levels"] = st["part_levels"]; out[k]["n_hits"] = st["n_hits"]
                    continue
                out[k]["ms_total"].append(round(st["ms_total"], 3)); out[k]["ms_scan"].append(round(st["ms_scan"], 3))
for k in kinds:
    out[k]["median_ms_total"] = statistics.median(out[k]["ms_total"])
    out[k]["median_ms_scan"] = statistics.median(out[k]["ms_scan"])
print(json.dumps(out))
