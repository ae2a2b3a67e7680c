"""The search rule of kg_proteins_search (include/kmerguts_hip.h) restated: the shared-k-mer counts as plain loops over sets of
windows and as sorted numpy arrays, then the candidates, the alignment (align_model) and the output order.  The GPU tests compare
the device's bytes with search_model (the numpy counts); the CPU tests compare the two forms with each other and with answers
worked out by hand."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import ALPHA, GAP_EXTEND, GAP_OPEN, MIN_RATIO_PCT

import align_model as AM
import cluster_model as M

K = M.K
MIN_SHARED, MAX_CAND, MAX_DB_PER_KMER = 2, 8, 256
COUNT_KEYS = ("targets", "queries", "valid_windows", "pairs", "kmers", "kmers_joined", "kmers_masked", "join_pairs")
STAT_KEYS = COUNT_KEYS + ("candidates", "aligned", "hits", "skipped", "queries_hit", "cells")


def shared_loops(seq: bytes, offsets, n_db: int, max_db_per_kmer: int = MAX_DB_PER_KMER):
    """-> ({(q, d): s}, counts).  The header's words, one window at a time."""
    seq = bytes(seq)
    n = len(offsets) - 1
    code = set(ALPHA)
    D, Q, valid, pairs = {}, {}, 0, 0
    for p in range(n):
        s = seq[offsets[p]:offsets[p + 1]]
        own = set()
        for i in range(0, len(s) - K):
            w = s[i:i + K]
            if any(ch not in code for ch in w):
                continue
            valid += 1
            own.add(w)
        pairs += len(own)
        for w in own:
            (D if p < n_db else Q).setdefault(w, []).append(p if p < n_db else p - n_db)
    s_of, joined, masked, join_pairs = {}, 0, 0, 0
    for w, ds in D.items():
        if len(ds) > max_db_per_kmer:
            masked += 1
            continue
        qs = Q.get(w, ())
        if not qs:
            continue
        joined += 1
        join_pairs += len(ds) * len(qs)
        for q in qs:
            for d in ds:
                s_of[(q, d)] = s_of.get((q, d), 0) + 1
    counts = dict(targets=n_db, queries=n - n_db, valid_windows=valid, pairs=pairs, kmers=len(set(D) | set(Q)), kmers_joined=joined,
                  kmers_masked=masked, join_pairs=join_pairs)
    return s_of, counts


def kmer_pairs(seq: bytes, offsets):
    """-> (k-mer numbers, protein indices) of every valid window, and their count; k-mers in base 20, most significant first."""
    seq = bytes(seq)
    n = len(offsets) - 1
    c = AM.codes(seq)
    L = len(c)
    if L <= K:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(c, K)             # windows at every position of the concatenation
    off = np.asarray(offsets, dtype=np.int64)
    length = np.diff(off)
    prot = np.repeat(np.arange(n), length)
    pos = np.arange(L) - off[prot]
    at = np.flatnonzero(pos < length[prot] - K)                      # positions [0, len_p - 8) of their own protein
    at = at[at < len(win)]
    w = win[at]
    ok = (w < 20).all(axis=1)
    v = (w[ok] * (20 ** np.arange(K - 1, -1, -1, dtype=np.int64))).sum(axis=1)
    return v, prot[at][ok]


def shared_numpy(seq: bytes, offsets, n_db: int, max_db_per_kmer: int = MAX_DB_PER_KMER):
    """The same by sorted arrays: distinct (k-mer, protein) pairs, the runs of a k-mer split at n_db, the cross product of each
    joined run, the distinct (q, d) counted."""
    n = len(offsets) - 1
    v, p = kmer_pairs(seq, offsets)
    counts = dict(targets=n_db, queries=n - n_db, valid_windows=int(v.size), pairs=0, kmers=0, kmers_joined=0, kmers_masked=0,
                  join_pairs=0)
    if v.size == 0:
        return {}, counts
    key = np.unique(v * (n + 1) + p)                                 # sorted distinct pairs: k-mer major, protein minor
    kv, kp = key // (n + 1), key % (n + 1)
    counts["pairs"] = int(key.size)
    head = np.flatnonzero(np.r_[True, kv[1:] != kv[:-1]])
    start = np.r_[head, key.size]
    counts["kmers"] = int(head.size)
    nd = np.add.reduceat((kp < n_db).astype(np.int64), head)
    nq = np.diff(start) - nd
    counts["kmers_masked"] = int((nd > max_db_per_kmer).sum())
    use = np.flatnonzero((nd >= 1) & (nd <= max_db_per_kmer) & (nq >= 1))
    counts["kmers_joined"] = int(use.size)
    w = nd[use] * nq[use]
    counts["join_pairs"] = int(w.sum())
    if use.size == 0:
        return {}, counts
    run = np.repeat(np.arange(use.size), w)
    t = np.arange(int(w.sum())) - np.repeat(np.cumsum(w) - w, w)
    d = kp[start[use][run] + t % nd[use][run]]
    q = kp[start[use][run] + nd[use][run] + t // nd[use][run]] - n_db
    qd, s = np.unique(q * (n_db + 1) + d, return_counts=True)
    return {(int(k // (n_db + 1)), int(k % (n_db + 1))): int(c) for k, c in zip(qd, s)}, counts


def candidates(s_of, n_q: int, min_shared: int = MIN_SHARED, max_cand: int = MAX_CAND):
    """-> per query the (d, s) that are aligned: s >= min_shared, larger s first, then smaller d, the first max_cand; and the
    number of candidates before the cut."""
    per = [[] for _ in range(n_q)]
    for (q, d), s in s_of.items():
        if s >= min_shared:
            per[q].append((d, s))
    total = sum(len(x) for x in per)
    return [sorted(x, key=lambda ds: (-ds[1], ds[0]))[:max_cand] for x in per], total


def search_model(seq: bytes, offsets, n_db: int, min_shared: int = MIN_SHARED, max_cand: int = MAX_CAND,
                 max_db_per_kmer: int = MAX_DB_PER_KMER, min_ratio_pct: int = MIN_RATIO_PCT, ref="longer", gap_open: int = GAP_OPEN,
                 gap_extend: int = GAP_EXTEND, max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, matrix=None, sw=AM.sw_numpy,
                 shared=shared_numpy):
    """-> (SEARCH_HIT_DTYPE records in (query, rank) order, hit_start int64[n_q + 1], the counts of kg_search_stats)."""
    S = AM.S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    ref = N.ALIGN_REFS.get("member" if ref == "query" else ref, ref)
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    n_q = n - n_db
    s_of, counts = shared(seq, offsets, n_db, max_db_per_kmer)
    per, counts["candidates"] = candidates(s_of, n_q, min_shared, max_cand)
    pairs = [(n_db + q, d) for q in range(n_q) for d, _ in per[q]]
    aln = AM.align_model(seq, offsets, pairs, S, gap_open, gap_extend, max_cells, sw)
    hits = np.zeros(len(pairs), dtype=N.SEARCH_HIT_DTYPE)
    start = np.zeros(n_q + 1, dtype=np.int64)
    counts.update(aligned=0, hits=0, skipped=0, queries_hit=0, cells=0)
    k = 0
    for q in range(n_q):
        recs = []
        for d, s in per[q]:
            a = aln[k]
            k += 1
            r = int(a["self_a"]) if ref == N.ALIGN_REF_MEMBER else max(int(a["self_a"]), int(a["self_b"]))
            if a["status"] == N.ALIGN_SKIPPED:
                status = N.SEARCH_SKIPPED
                counts["skipped"] += 1
            else:
                status = N.SEARCH_HIT if AM.kept(int(a["score"]), r, min_ratio_pct) else N.SEARCH_BELOW
                counts["aligned"] += 1
                counts["hits"] += status == N.SEARCH_HIT
                counts["cells"] += int(offsets[n_db + q + 1] - offsets[n_db + q]) * int(offsets[d + 1] - offsets[d])
            recs.append((q, d, s, int(a["score"]), int(a["self_a"]), int(a["self_b"]), int(a["end_a"]), int(a["end_b"]), status))
        # not skipped first, then larger score, then larger s, then smaller target
        recs.sort(key=lambda x: (x[8] == N.SEARCH_SKIPPED, -x[3], -x[2], x[1]))
        for rank, x in enumerate(recs):
            hits[start[q] + rank] = x + (rank,)
        start[q + 1] = start[q] + len(recs)
        counts["queries_hit"] += bool(recs) and recs[0][8] == N.SEARCH_HIT
    counts = {key: int(v) for key, v in counts.items()}
    return hits, start, counts


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------

def batch(proteins):
    """-> (seq bytes, offsets int64[n + 1]) of a list of bytes."""
    off = np.zeros(len(proteins) + 1, dtype=np.int64)
    if proteins:
        off[1:] = np.cumsum([len(p) for p in proteins])
    return b"".join(proteins), off


def distinct_kmers(rng, count: int, avoid=()):
    """`count` 8-mers (bytes) that differ from each other and from `avoid`, none sharing an 8-mer with another by overlap when
    they are joined with the spacer below."""
    seen, out = set(avoid), []
    while len(out) < count:
        w = bytes(ALPHA[int(x)] for x in rng.integers(0, 20, K))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


SPACER = b"X"       # between planted 8-mers: no window crosses it, and a protein needs one more residue than its last window


def protein_of(kmers) -> bytes:
    """A protein whose valid windows are exactly the given 8-mers: each followed by a non-residue."""
    return b"".join(w + SPACER for w in kmers)
