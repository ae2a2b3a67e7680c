"""The rule of kg_contigs_search_translated (include/kmerguts_hip.h, "genes by homology") restated in Python: the exact reference
the GPU tests compare against, byte for byte.  `calls_of` is a plain loop over rule 3; `translated_model` is the whole call out of
the models of its parts: free_orfs_model.free_orfs with start_codons = 0, trace_model.search_paths_model on "the targets, then
the fragments' proteins", then calls_of."""
from __future__ import annotations

import numpy as np

import free_orfs_model as F
import trace_model as T
from kmergutsjava_amd import _native as N

MIN_RES, MAX_HITS = N.TRANSLATE_MIN_RES, N.TRANSLATE_MAX_HITS
DROPS = ("dropped_status", "dropped_rank", "dropped_untraced")


def first_codon(frag, L: int) -> int:
    """Rule 1: b, the fragment's first codon in its frame."""
    x = int(frag["left"]) if int(frag["strand"]) == 0 else L - 1 - int(frag["right"])
    return (x - int(frag["frame"])) // 3


def calls_of(frags, hits, paths, offsets, max_hits: int = MAX_HITS, target_fn=None):
    """frags ORF_DTYPE (fragment q is query q), hits SEARCH_HIT_DTYPE with paths ALIGN_PATH_DTYPE of the same indices, offsets the
    contigs' -> (CALL_DTYPE records, call_hit int64, the three drop counts)."""
    off = [int(x) for x in offsets]
    calls, call_hit = [], []
    drops = dict.fromkeys(DROPS, 0)
    for r in range(len(hits)):
        h, p = hits[r], paths[r]
        if int(h["status"]) != N.SEARCH_HIT:
            drops["dropped_status"] += 1
            continue
        if int(h["rank"]) >= max_hits:
            drops["dropped_rank"] += 1
            continue
        if int(p["status"]) != N.PATH_TRACED:
            drops["dropped_untraced"] += 1
            continue
        f = frags[int(h["query"])]
        s = int(f["seq"])
        b = first_codon(f, off[s + 1] - off[s])
        fi = int(h["target"]) if target_fn is None else int(target_fn[int(h["target"])])
        calls.append((6 * s + 3 * int(f["strand"]) + int(f["frame"]), b + int(p["start_a"]), b + int(h["end_query"]), int(h["score"]), fi,
                      np.float32(int(h["score"]))))
        call_hit.append(r)
    out = np.zeros(len(calls), dtype=N.CALL_DTYPE)
    for k, c in enumerate(calls):
        out[k] = c
    return out, np.asarray(call_hit, dtype=np.int64), drops


def translated_model(seq, offsets, target_seq: bytes, target_offsets, min_res: int = MIN_RES, max_hits: int = MAX_HITS, target_fn=None,
                     max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, **search):
    """seq / offsets: the contigs; target_seq / target_offsets: the database; search: search_model's keywords.
    -> dict(fragments=(records, prot_start, residues), hits, hit_start, paths, calls, call_hits, drops)."""
    frags, pstart, res = F.free_orfs(seq, offsets, min_res=min_res, start_codons=0)
    toff = np.asarray(target_offsets, dtype=np.int64)
    n_db = toff.size - 1
    tseq = bytes(target_seq)[int(toff[0]):int(toff[-1])]
    both = tseq + res.tobytes()
    boff = np.concatenate([toff - toff[0], (toff[-1] - toff[0]) + pstart[1:]])
    hits, start, paths, _counts = T.search_paths_model(both, boff, n_db, paths="hits", max_trace_cells=max_trace_cells, **search)
    calls, call_hits, drops = calls_of(frags, hits, paths, offsets, max_hits, target_fn)
    return dict(fragments=(frags, pstart, res), hits=hits, hit_start=start, paths=paths, calls=calls, call_hits=call_hits, drops=drops)
