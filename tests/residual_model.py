"""The rule of kg_contigs_search_residual (include/kmerguts_hip.h, "signature and homology evidence in one run") restated in
Python with plain loops: the exact reference the tests compare against, byte for byte.  `explain_of` is rule 2, `merge_of` rules 5
(the cut) and 6; `residual_model` is the whole call out of the models of its parts: free_orfs_model.free_orfs with
start_codons = 0, explain_of, trace_model.search_paths_model on "the targets, then the searched fragments' proteins",
translated_model.calls_of, merge_of."""
from __future__ import annotations

import numpy as np

import free_orfs_model as F
import trace_model as T
import translated_model as TM
from kmergutsjava_amd import _native as N


def explain_of(frags, off, sig_calls):
    """frags ORF_DTYPE, off the contigs' offsets, sig_calls CALL_DTYPE -> explain int64[len(frags)] (rule 2)."""
    off = [int(x) for x in off]
    calls = [(int(c["container"]), int(c["start"]), int(c["end"]), int(c["count"])) for c in sig_calls]
    explain = np.zeros(len(frags), dtype=np.int64)
    for k, f in enumerate(frags):
        s = int(f["seq"])
        c = 6 * s + 3 * int(f["strand"]) + int(f["frame"])
        b = TM.first_codon(f, off[s + 1] - off[s])
        last = b + int(f["n_res"]) - 1
        total = 0
        for container, start, end, count in calls:
            if container == c and start <= last and end >= b:
                total += count
        explain[k] = total
    return explain


def subset_of(frags, pstart, res, explain, explain_min: int = 1):
    """Rule 3 -> (searched int64, records, prot_start, residues) of the fragments with explain < explain_min."""
    searched = [k for k in range(len(frags)) if int(explain[k]) < explain_min]
    new_start = [0]
    pieces = []
    for k in searched:
        pieces.append(res[int(pstart[k]):int(pstart[k + 1])])
        new_start.append(new_start[-1] + len(pieces[-1]))
    out = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    return np.asarray(searched, dtype=np.int64), frags[searched].copy(), np.asarray(new_start, dtype=np.int64), out.astype(np.uint8)


def merge_of(sig_calls, db_calls, db_hits, min_db_count: int = 0):
    """Rules 5 (the cut) and 6 -> (merged CALL_DTYPE, call_kind uint8, call_source int64, call_hit int64, dropped)."""
    items = []          # (container, kind, source)
    dropped = 0
    for i in range(len(sig_calls)):
        items.append((int(sig_calls[i]["container"]), 0, i))
    for j in range(len(db_calls)):
        if int(db_calls[j]["count"]) < min_db_count:
            dropped += 1
            continue
        items.append((int(db_calls[j]["container"]), 1, j))
    items.sort()        # by container, signature first, then the list's own order
    merged = np.zeros(len(items), dtype=N.CALL_DTYPE)
    kind = np.zeros(len(items), dtype=np.uint8)
    source = np.zeros(len(items), dtype=np.int64)
    hit = np.zeros(len(items), dtype=np.int64)
    for k, (_c, kd, src) in enumerate(items):
        merged[k] = sig_calls[src] if kd == 0 else db_calls[src]
        kind[k], source[k] = kd, src
        hit[k] = -1 if kd == 0 else int(db_hits[src])
    return merged, kind, source, hit, dropped


def residual_model(seq, offsets, target_seq: bytes, target_offsets, sig_calls, target_fn, min_res: int = TM.MIN_RES,
                   max_hits: int = TM.MAX_HITS, explain_min: int = 1, min_db_count: int = 0,
                   max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, **search):
    """-> dict(fragments, explain, searched, searched_fragments, hits, hit_start, paths, db_calls, db_hits, drops, calls, call_kind,
    call_source, call_hits, dropped_min_count)."""
    frags, pstart, res = F.free_orfs(seq, offsets, min_res=min_res, start_codons=0)
    explain = explain_of(frags, offsets, sig_calls)
    searched, recs, nstart, nres = subset_of(frags, pstart, res, explain, explain_min)
    toff = np.asarray(target_offsets, dtype=np.int64)
    n_db = toff.size - 1
    tseq = bytes(target_seq)[int(toff[0]):int(toff[-1])]
    both = tseq + nres.tobytes()
    boff = np.concatenate([toff - toff[0], (toff[-1] - toff[0]) + nstart[1:]])
    hits, start, paths, _counts = T.search_paths_model(both, boff, n_db, paths="hits", max_trace_cells=max_trace_cells, **search)
    db_calls, db_hits, drops = TM.calls_of(recs, hits, paths, offsets, max_hits, target_fn)
    calls, kind, source, hit, dropped = merge_of(sig_calls, db_calls, db_hits, min_db_count)
    return dict(fragments=(frags, pstart, res), explain=explain, searched=searched, searched_fragments=(recs, nstart, nres), hits=hits,
                hit_start=start, paths=paths, db_calls=db_calls, db_hits=db_hits, drops=drops, calls=calls, call_kind=kind,
                call_source=source, call_hits=hit, dropped_min_count=dropped)


def evidence_of(regions, calls, call_kind, offsets):
    """The front end's `evidence` field: per region "table", "db" or "table+db", from the kinds of the CALLs of its (seq, strand,
    fI) group whose x0 = frame + 3 * start lies inside it ('-': mirrored into contig coordinates)."""
    off = [int(x) for x in offsets]
    out = []
    for r in regions:
        kinds = set()
        for c, kd in zip(calls, call_kind):
            cont = int(c["container"])
            s, strand, frame = cont // 6, (cont % 6) // 3, cont % 3
            if s != int(r["seq"]) or strand != int(r["strand"]) or int(c["fI"]) != int(r["fI"]):
                continue
            L = off[s + 1] - off[s]
            x0 = frame + 3 * int(c["start"])
            pos = x0 if strand == 0 else L - 1 - x0
            if int(r["left"]) <= pos <= int(r["right"]):
                kinds.add(int(kd))
        out.append("table+db" if kinds == {0, 1} else "db" if kinds == {1} else "table")
    return out
