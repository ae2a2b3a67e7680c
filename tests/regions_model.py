"""The region rule of kg_result_regions / kg_regions_calls (include/kmerguts_hip.h) restated in numpy: the exact reference the
GPU tests compare against, byte for byte.  Imports nothing from kmergutsjava_amd but the record dtypes."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import CALL_DTYPE, REGION_DTYPE


def spans(calls, offsets):
    """Rule 1: (seq, strand, frame, x0, x1, L) of every CALL, all int64."""
    c = np.asarray(calls, dtype=CALL_DTYPE)
    off = np.asarray(offsets, dtype=np.int64)
    cont = c["container"].astype(np.int64)
    seq, k = cont // 6, cont % 6
    strand, frame = (k >= 3).astype(np.int64), k % 3
    x0 = frame + 3 * c["start"].astype(np.int64)
    x1 = frame + 3 * c["end"].astype(np.int64) + 2
    L = off[seq + 1] - off[seq] if c.size else np.zeros(0, np.int64)
    return seq, strand, frame, x0, x1, L


def _sorted_out(regs, n_seqs):
    order = np.lexsort((regs["fI"], regs["strand"], regs["right"], regs["left"], regs["seq"]))
    regs = regs[order]
    start = np.searchsorted(regs["seq"], np.arange(n_seqs + 1), side="left").astype(np.int64)
    return regs, start


def regions(calls, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0):
    """calls CALL_DTYPE in calls[] order, offsets int64[n_seqs + 1] -> (REGION_DTYPE records in output order,
    region_start int64[n_seqs + 1])."""
    c = np.asarray(calls, dtype=CALL_DTYPE)
    off = np.asarray(offsets, dtype=np.int64)
    n_seqs = off.size - 1
    n = c.size
    if n == 0:
        return np.zeros(0, REGION_DTYPE), np.zeros(n_seqs + 1, np.int64)
    seq, strand, frame, x0, x1, L = spans(c, off)
    assert (x0 >= 0).all() and (x0 <= x1).all() and (x1 <= L - 1).all() and (seq < n_seqs).all()
    fI = c["fI"].astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    order = np.lexsort((idx, x0, fI, strand, seq))            # rule 2: group order
    seq, strand, frame, x0, x1, L, fI, idx = (a[order] for a in (seq, strand, frame, x0, x1, L, fI, idx))
    cnt = c["count"].astype(np.int64)[order]
    wt = c["weightedHits"].astype(np.float32)[order]
    ghead = np.ones(n, dtype=bool)
    ghead[1:] = (seq[1:] != seq[:-1]) | (strand[1:] != strand[:-1]) | (fI[1:] != fI[:-1])
    g = np.cumsum(ghead) - 1
    # rule 3: the largest x1 so far in the group (= in the region: a CALL that opens one starts behind every earlier end)
    run = np.maximum.accumulate(g * (1 << 32) + x1)
    rmax = run & 0xFFFFFFFF
    rhead = ghead.copy()
    rhead[1:] |= (x0[1:] - rmax[:-1] - 1) > merge_gap
    first = np.flatnonzero(rhead)
    last = np.concatenate([first[1:], [n]]) - 1
    rid = np.cumsum(rhead) - 1
    m = first.size
    out = np.zeros(m, dtype=REGION_DTYPE)
    lo, R, Ls, st = x0[first], rmax[last], L[first], strand[first]
    out["seq"], out["strand"], out["fI"] = seq[first], st, fI[first]
    out["left"] = np.where(st == 0, lo, Ls - 1 - R)
    out["right"] = np.where(st == 0, R, Ls - 1 - lo)
    score = np.add.reduceat(cnt, first)
    assert (score < 2 ** 31).all()
    out["score"] = score
    out["n_calls"] = last - first + 1
    out["frames"] = np.bitwise_or.reduceat(1 << frame, first)
    out["first_call"] = idx[first]
    # weighted: float32 adds in group order, the j-th CALL of every region at step j
    pos = np.arange(n) - first[rid]
    W = np.zeros(m, dtype=np.float32)
    by_pos = np.argsort(pos, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(pos))])
    for j in range(bounds.size - 1):
        sel = by_pos[bounds[j]:bounds[j + 1]]
        W[rid[sel]] = W[rid[sel]] + wt[sel]
    out["weighted"] = W
    # best_frame: the largest count, ties to the first in group order
    best = np.lexsort((pos, -cnt, rid))
    out["best_frame"] = frame[best[np.flatnonzero(np.concatenate([[True], rid[best][1:] != rid[best][:-1]]))]]
    out["kept"] = ((score >= min_score) & (out["right"].astype(np.int64) - out["left"] + 1 >= min_len)).astype(np.int32)
    return _sorted_out(out, n_seqs)


def brute_force(calls, offsets, merge_gap: int = 600, min_score: int = 0, min_len: int = 0):
    """The same rule one contig at a time, with plain loops."""
    off = [int(x) for x in offsets]
    n_seqs = len(off) - 1
    per = [[] for _ in range(n_seqs)]
    for i, r in enumerate(calls):
        per[int(r["container"]) // 6].append(i)
    recs = []
    for s in range(n_seqs):
        L = off[s + 1] - off[s]
        groups = {}
        for i in per[s]:
            r = calls[i]
            k = int(r["container"]) % 6
            f = k % 3
            groups.setdefault((k // 3, int(r["fI"])), []).append((f + 3 * int(r["start"]), i, f + 3 * int(r["end"]) + 2, f))
        for (strand, fi), items in groups.items():
            items.sort()
            cur = None
            for x0, i, x1, f in items:
                if cur is None or x0 - cur["R"] - 1 > merge_gap:
                    cur = {"lo": x0, "R": x1, "score": 0, "w": np.float32(0), "n": 0, "frames": 0, "best": (-1, 0), "first": i,
                           "strand": strand, "fI": fi}
                    recs.append((s, L, cur))
                cur["R"] = max(cur["R"], x1)
                cur["score"] += int(calls[i]["count"])
                cur["w"] = np.float32(cur["w"] + np.float32(calls[i]["weightedHits"]))
                cur["n"] += 1
                cur["frames"] |= 1 << f
                if int(calls[i]["count"]) > cur["best"][0]:
                    cur["best"] = (int(calls[i]["count"]), f)
    out = np.zeros(len(recs), dtype=REGION_DTYPE)
    for k, (s, L, r) in enumerate(recs):
        left, right = (r["lo"], r["R"]) if r["strand"] == 0 else (L - 1 - r["R"], L - 1 - r["lo"])
        out[k] = (s, r["strand"], left, right, r["fI"], r["score"], r["w"], r["n"], r["frames"], r["best"][1], r["first"],
                  int(r["score"] >= min_score and right - left + 1 >= min_len))
    return _sorted_out(out, n_seqs)


def random_calls(rng, n_seqs: int, max_calls: int = 8, n_fn: int = 3, max_len: int = 400, span: int = 30):
    """Random valid CALL lists built for collisions: few functions, short contigs, equal x0 across frames, nested and
    abutting CALLs.  -> (calls in container order, offsets)."""
    lens = rng.integers(0, max_len + 1, size=n_seqs)
    off = np.zeros(n_seqs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    rows = []
    for s in range(n_seqs):
        L = int(lens[s])
        for _ in range(int(rng.integers(0, max_calls + 1)) if L >= 3 else 0):
            k = int(rng.integers(0, 6))
            f = k % 3
            res = (L - f) // 3                     # complete codons of this frame
            if res < 1:
                continue
            a = int(rng.integers(0, res))
            b = min(res - 1, a + int(rng.integers(0, span + 1)) * int(rng.choice([0, 1, 1, 4])))
            rows.append((6 * s + k, a, b, int(rng.integers(0, 7)), int(rng.integers(0, n_fn)) - 1,
                         float(rng.choice(np.array([0.5, 1.0, 1.25, 2.0, 3.0, 0.1, 2.0 ** 24], np.float32)))))
    rows.sort(key=lambda r: r[0])                  # stable: emission order inside a container is the draw order
    calls = np.zeros(len(rows), dtype=CALL_DTYPE)
    for i, r in enumerate(rows):
        calls[i] = r
    return calls, off


def random_calls_large(rng, n_seqs: int, n_calls: int, n_fn: int, contig_len: int = 30_000, span: int = 120):
    """The same in vectorised form for large lists: contigs of one length."""
    off = np.arange(n_seqs + 1, dtype=np.int64) * contig_len
    cont = np.sort(rng.integers(0, 6 * n_seqs, size=n_calls)).astype(np.uint32)
    f = (cont % 6) % 3
    res = (contig_len - f) // 3
    a = rng.integers(0, res)
    b = np.minimum(res - 1, a + rng.integers(0, span + 1, size=n_calls))
    calls = np.zeros(n_calls, dtype=CALL_DTYPE)
    calls["container"], calls["start"], calls["end"] = cont, a, b
    calls["count"] = rng.integers(0, 40, size=n_calls)
    calls["fI"] = rng.integers(0, n_fn, size=n_calls)
    calls["weightedHits"] = rng.choice(np.array([0.5, 1.0, 1.25, 2.0, 3.0, 0.1, 2.0 ** 24], np.float32), size=n_calls)
    return calls, off
