"""The ungapped filter of kg_proteins_search_filtered (include/kmerguts_hip.h) restated twice: as plain loops over windows,
seeds and cells, and as sorted numpy arrays.  Both forms give, per candidate, s, the best seed diagonal g*, m(g*) and u; the cut
and everything behind it is search_model's (the alignment is align_model's).  The seeds are seed_model's: the exact call is its
EXACT seed set, whose windows are the derive windows.  The GPU tests compare the device's bytes with filtered_model; the CPU tests
compare the two forms with each other and with answers worked out by hand."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N

import align_model as AM
import search_model as SM
import seed_model as SD

UNGAPPED_KEYS = ("scored", "dropped", "cut", "cells")


# ---- positions: i_p(v), the smallest valid window position of seed id v in protein p -------------------------------------------

def first_positions_loops(p: bytes, seed) -> dict:
    """The rule one window at a time: {seed id: its smallest valid window position in p}."""
    cls, masks = seed
    A, w = SD.alphabet_size(cls), SD.weight(masks[0])
    code = {ch: k for k, ch in enumerate(SD.ALPHA)}
    out = {}
    for k, mask in enumerate(masks):
        care = [j for j in range(32) if mask >> j & 1]
        for i in range(len(p)):
            if not i + SD.span(mask) < len(p) or any(p[i + j] not in code for j in care):
                continue
            value = 0
            for j in care:
                value = value * A + cls[code[p[i + j]]]
            v = k * A ** w + value
            if v not in out:
                out[v] = i
    return out


def first_positions_numpy(seq: bytes, offsets, seed):
    """-> (seed ids, proteins, first positions) of the distinct (seed id, protein) pairs, seed id major and protein minor."""
    cls, masks = seed
    A, w = SD.alphabet_size(cls), SD.weight(masks[0])
    seq = bytes(seq)
    n = len(offsets) - 1
    c = AM.codes(seq)
    off = np.asarray(offsets, dtype=np.int64)
    length = np.diff(off)
    prot = np.repeat(np.arange(n), length)
    pos = np.arange(len(c)) - off[prot]                     # (offsets[0] = 0, as in seed_model.seed_pairs)
    klass = np.r_[np.asarray(cls, dtype=np.int64), -1][np.minimum(c, 20)]
    vs, ps, xs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for k, mask in enumerate(masks):
        care = np.array([j for j in range(32) if mask >> j & 1], dtype=np.int64)
        at = np.flatnonzero(pos + SD.span(mask) < length[prot])
        if at.size == 0:
            continue
        digits = klass[at[:, None] + care[None, :]]
        ok = (digits >= 0).all(axis=1)
        vs.append(k * A ** w + (digits[ok] * (A ** np.arange(w - 1, -1, -1, dtype=np.int64))).sum(axis=1))
        ps.append(prot[at][ok])
        xs.append(pos[at][ok])
    v, p, x = np.concatenate(vs), np.concatenate(ps), np.concatenate(xs)
    order = np.lexsort((x, p, v))
    v, p, x = v[order], p[order], x[order]
    head = np.r_[True, (v[1:] != v[:-1]) | (p[1:] != p[:-1])] if v.size else np.zeros(0, dtype=bool)
    return v[head], p[head], x[head]


# ---- diagonals: per candidate s, g* and m(g*) ------------------------------------------------------------------------------------

def best_of(diagonals):
    """[g of every shared seed] -> (s, g*, m(g*)): the diagonal with the most seeds, on a tie the smallest."""
    m = {}
    for g in diagonals:
        m[g] = m.get(g, 0) + 1
    g_star = min(m, key=lambda g: (-m[g], g))
    return len(diagonals), g_star, m[g_star]


def diagonals_loops(seeding: bytes, offsets, n_db: int, seed, max_db_per_kmer: int = SM.MAX_DB_PER_KMER) -> dict:
    """{(q, d): (s, g*, m)} of every pair that shares an unmasked seed, the header's words one seed at a time.  seeding: the
    bytes the window pass reads (the masked copy under a mask)."""
    seeding = bytes(seeding)
    n = len(offsets) - 1
    first = [first_positions_loops(seeding[offsets[p]:offsets[p + 1]], seed) for p in range(n)]
    D, Q = {}, {}
    for p in range(n):
        for v in first[p]:
            (D if p < n_db else Q).setdefault(v, []).append(p)
    diag = {}
    for v, ds in D.items():
        if len(ds) > max_db_per_kmer:
            continue
        for q in Q.get(v, ()):
            for d in ds:
                diag.setdefault((q - n_db, d), []).append(first[q][v] - first[d][v])
    return {qd: best_of(gs) for qd, gs in diag.items()}


def diagonals_numpy(seeding: bytes, offsets, n_db: int, seed, max_db_per_kmer: int = SM.MAX_DB_PER_KMER) -> dict:
    """The same by sorted arrays: the runs of a seed id split at n_db, the cross product of each joined run with its diagonals,
    the (q, d, g) triples counted and the best of each (q, d) taken by a sort."""
    v, p, x = first_positions_numpy(seeding, offsets, seed)
    if v.size == 0:
        return {}
    head = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
    start = np.r_[head, v.size]
    nd = np.add.reduceat((p < n_db).astype(np.int64), head)
    nq = np.diff(start) - nd
    use = np.flatnonzero((nd >= 1) & (nd <= max_db_per_kmer) & (nq >= 1))
    if use.size == 0:
        return {}
    wt = nd[use] * nq[use]
    run = np.repeat(np.arange(use.size), wt)
    t = np.arange(int(wt.sum())) - np.repeat(np.cumsum(wt) - wt, wt)
    at_d = start[use][run] + t % nd[use][run]
    at_q = start[use][run] + nd[use][run] + t // nd[use][run]
    q, d, g = p[at_q] - n_db, p[at_d], x[at_q] - x[at_d]
    order = np.lexsort((g, d, q))
    q, d, g = q[order], d[order], g[order]
    ghead = np.flatnonzero(np.r_[True, (q[1:] != q[:-1]) | (d[1:] != d[:-1]) | (g[1:] != g[:-1])])
    m = np.diff(np.r_[ghead, q.size])
    gq, gd, gg = q[ghead], d[ghead], g[ghead]
    best = np.lexsort((gg, -m, gd, gq))                     # inside a (q, d): larger m first, then smaller g
    gq, gd, gg, m = gq[best], gd[best], gg[best], m[best]
    phead = np.flatnonzero(np.r_[True, (gq[1:] != gq[:-1]) | (gd[1:] != gd[:-1])])
    s = np.add.reduceat(m, phead)
    return {(int(a), int(b)): (int(c), int(e), int(f)) for a, b, c, e, f in zip(gq[phead], gd[phead], s, gg[phead], m[phead])}


# ---- the ungapped score of one diagonal ------------------------------------------------------------------------------------------

def cells_of(len_q: int, len_d: int, g: int) -> int:
    """The number of cells (a, a - g) with 0 <= a < len_q and 0 <= a - g < len_d."""
    return max(min(len_q, len_d + g) - max(g, 0), 0)


def ungapped_loops(a: bytes, b: bytes, g: int, S=AM.S62) -> int:
    """u: the largest sum over a non-empty run of consecutive cells of diagonal g, 0 if every run is negative.  One cell at a time."""
    ca, cb = [int(x) for x in AM.codes(a)], [int(x) for x in AM.codes(b)]
    best = run = 0
    for i in range(len(ca)):
        j = i - g
        if 0 <= j < len(cb):
            run = max(run, 0) + int(S[ca[i]][cb[j]])
            best = max(best, run)
    return best


def ungapped_numpy(a: bytes, b: bytes, g: int, S=AM.S62) -> int:
    """The same as max_j (P_j - min_{i < j} P_i) over the prefix sums P of the cells, P_{-1} = 0."""
    a0, a1 = max(g, 0), min(len(a), len(b) + g)
    if a1 <= a0:
        return 0
    cell = np.asarray(S, dtype=np.int64)[AM.codes(a[a0:a1]), AM.codes(b[a0 - g:a1 - g])]
    P = np.cumsum(cell)
    low = np.minimum.accumulate(np.r_[0, P[:-1]])
    return max(int((P - low).max()), 0)


# ---- the whole call --------------------------------------------------------------------------------------------------------------

def scored(seq: bytes, offsets, n_db: int, seed=None, seeding=None, min_shared: int = SM.MIN_SHARED,
           max_db_per_kmer: int = SM.MAX_DB_PER_KMER, matrix=None, form: str = "numpy") -> dict:
    """{(q, d): (s, g*, m, u)} of every candidate (s >= min_shared).  seeding: the bytes the window pass reads, the original by
    default; the scores are read from seq."""
    seq = bytes(seq)
    S = AM.S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    diag = (diagonals_numpy if form == "numpy" else diagonals_loops)(seq if seeding is None else seeding, offsets, n_db,
                                                                     SD.EXACT if seed is None else seed, max_db_per_kmer)
    u_of = ungapped_numpy if form == "numpy" else ungapped_loops
    out = {}
    for (q, d), (s, g, m) in diag.items():
        if s >= min_shared:
            a, b = seq[offsets[n_db + q]:offsets[n_db + q + 1]], seq[offsets[d]:offsets[d + 1]]
            out[(q, d)] = (s, g, m, u_of(a, b, g, S))
    return out


def cut(cands: dict, n_q: int, min_ungapped: int = 0, max_cand: int = SM.MAX_CAND):
    """-> per query the (d, s, g, m, u) that are aligned: u >= min_ungapped, larger u first, then larger s, then smaller d, the
    first max_cand; and (dropped, cut)."""
    per = [[] for _ in range(n_q)]
    dropped = 0
    for (q, d), (s, g, m, u) in cands.items():
        if u >= min_ungapped:
            per[q].append((d, s, g, m, u))
        else:
            dropped += 1
    kept = [sorted(x, key=lambda c: (-c[4], -c[1], c[0]))[:max_cand] for x in per]
    return kept, dropped, sum(len(x) for x in per) - sum(len(x) for x in kept)


def filtered_model(seq: bytes, offsets, n_db: int, seed=None, seeding=None, min_ungapped: int = 0, min_shared: int = SM.MIN_SHARED,
                   max_cand: int = SM.MAX_CAND, max_db_per_kmer: int = SM.MAX_DB_PER_KMER, matrix=None, form: str = "numpy", **kw):
    """-> (SEARCH_HIT_DTYPE records, hit_start, SEARCH_UNGAPPED_DTYPE records of the same indices, the counts of
    kg_search_stats, the counts of kg_ungapped_stats).  kw: search_model's alignment arguments."""
    seq = bytes(seq)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_q = len(offsets) - 1 - n_db
    seed_set = SD.EXACT if seed is None else seed
    cands = scored(seq, offsets, n_db, seed, seeding, min_shared, max_db_per_kmer, matrix, form)
    kept, dropped, n_cut = cut(cands, n_q, min_ungapped, max_cand)
    chosen = {(q, c[0]): c[1] for q in range(n_q) for c in kept[q]}
    inner = SD.shared_numpy(seed_set)

    def shared(_seq, offsets_, n_db_, max_db_per_kmer_=SM.MAX_DB_PER_KMER):
        _, counts = inner(seq if seeding is None else seeding, offsets_, n_db_, max_db_per_kmer_)
        return chosen, counts

    hits, start, counts = SM.search_model(seq, offsets, n_db, min_shared=1, max_cand=max(max_cand, 1), max_db_per_kmer=max_db_per_kmer,
                                          matrix=matrix, shared=shared, **kw)
    counts["candidates"] = len(cands)
    ung = np.zeros(len(hits), dtype=N.SEARCH_UNGAPPED_DTYPE)
    for k, h in enumerate(hits):
        s, g, m, u = cands[(int(h["query"]), int(h["target"]))]
        ung[k] = (u, g, m, 0)
    cells = sum(cells_of(int(offsets[n_db + q + 1] - offsets[n_db + q]), int(offsets[d + 1] - offsets[d]), g)
                for (q, d), (s, g, m, u) in cands.items())
    return hits, start, ung, counts, dict(scored=len(cands), dropped=dropped, cut=n_cut, cells=cells)
