"""Time and quality of composition binning on the GPU (kg_contigs_compose), one JSON line per measurement.

    python tools/compose_time.py [--reps 6] [--out profiles/compose_time.jsonl]

Inputs: the E. coli genome of tests/golden as one labelled contig (one model); a 100 Mbp synth contig mix (synth.contig_mix_lengths,
synth.random_dna) whose even contigs carry the labels 0 .. 63 in turn (64 models, min_train 0).
Per input and repetition:
  compose     count ms (the count pass, the fold, the label rows and their copy to the host), score ms, wall ms, and the count
              pass's bytes per second taken over count ms.
  background  the yardstick of the same run: coding_background_kernel on the same bytes, as the count ms of kg_orfset_coding on an
              ORF set without records (kg_orfs_free with a min_res no ORF reaches): the background pass and its fold.
The first repetition of an input carries the module load or the first allocations of its size: leave it out.
Quality, once: the E. coli genome cut into 5 kbp pieces against a synth genome of the same length with GC 0.35 (i.i.d. bases),
every other piece of each labelled, at the default parameters: correct, wrong and undecided among the unlabelled pieces.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import hotpath, synth  # noqa: E402
from kmergutsjava_amd.make_signatures import parse_fasta  # noqa: E402


def _emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def background_ms(lib, seq, off) -> float:
    none, scored = C.c_void_p(), C.c_void_p()
    args = (seq.ctypes.data, 0, off.ctypes.data, len(off) - 1)
    N.check(lib.kg_orfs_free(0, C.byref(N.KgFreeParams(1 << 30, 7, 0)), *args, C.byref(none)))
    try:
        assert lib.kg_orfset_count(none) == 0
        N.check(lib.kg_orfset_coding(none, C.byref(N.KgCodingParams(0, 0, 0)), None, *args, C.byref(scored)))
        try:
            st = N.KgCodingStats()
            N.check(lib.kg_orfset_coding_stats(scored, C.byref(st)))
        finally:
            lib.kg_orfset_free(scored)
    finally:
        lib.kg_orfset_free(none)
    return float(st.ms_count)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_time.jsonl"))
    a = ap.parse_args()
    import torch
    gpu = torch.cuda.get_device_name(0)
    lib = N.load()
    genome = parse_fasta(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.fna.gz"), "rb").read()))[1]
    ecoli = np.frombuffer(b"".join(genome), dtype=np.uint8)
    lens = synth.contig_mix_lengths(100_000_000)
    mix_labels = np.where(np.arange(len(lens)) % 2 == 0, (np.arange(len(lens)) // 2) % 64, -1).astype(np.int32)
    inputs = [("ecoli", ecoli, synth.offsets_of(np.array([len(c) for c in genome], np.int64)), np.zeros(len(genome), np.int32)),
              ("synth_mix_100mbp", synth.random_dna(100_000_000, 77).numpy(), synth.offsets_of(lens), mix_labels)]
    for name, seq, off, labels in inputs:
        base = {"input": name, "contigs": len(off) - 1, "nucleotides": int(off[-1]), "gpu": gpu}
        for rep in range(a.reps):
            st = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hotpath.compose_contigs(seq, off, labels, None, min_train=0, stats=st)
            wall = (time.perf_counter() - t0) * 1e3
            _emit(a.out, dict(base, what="compose", rep=rep, wall_ms=round(wall, 2), count_ms=round(st["ms_count"], 3),
                              score_ms=round(st["ms_score"], 3), models=st["models"], windows=st["windows"], decided=st["decided"],
                              count_gb_per_s=round(int(off[-1]) / st["ms_count"] / 1e6, 1)))
            ms = background_ms(lib, seq, off)
            _emit(a.out, dict(base, what="background", rep=rep, count_ms=round(ms, 3), count_gb_per_s=round(int(off[-1]) / ms / 1e6, 1)))
    # quality at the defaults
    rng = np.random.default_rng(11)
    other = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=len(ecoli), p=[0.325, 0.175, 0.175, 0.325])
    piece = 5000
    n_each = len(ecoli) // piece
    seq = np.concatenate([ecoli[:n_each * piece], other[:n_each * piece]])
    off = np.arange(2 * n_each + 1, dtype=np.int64) * piece
    truth = np.repeat(np.array([0, 1], np.int32), n_each)
    labels = np.where(np.arange(2 * n_each) % 2 == 0, truth, -1).astype(np.int32)
    st = {}
    cls = hotpath.compose_contigs(seq, off, labels, stats=st)["classes"]
    free = labels < 0
    dec = cls["decided"] != 0
    _emit(a.out, {"what": "quality", "pieces": int(2 * n_each), "piece_bp": piece, "unlabelled": int(free.sum()), "models": st["models"],
                  "correct": int((free & dec & (cls["best"] == truth)).sum()), "wrong": int((free & dec & (cls["best"] != truth)).sum()),
                  "undecided": int((free & ~dec).sum()), "conflicts": st["conflicts"], "gpu": gpu})
    return 0


if __name__ == "__main__":
    sys.exit(main())
