"""The assignment rule of kg_result_assign / kg_assign_calls (include/kmerguts_hip.h) restated in numpy: the exact reference
the GPU tests compare against, byte for byte.  Imports nothing from kmergutsjava_amd but the record dtypes."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import ASSIGNMENT_DTYPE, CALL_DTYPE, OTU_DTYPE


def _empty(n):
    out = np.zeros(n, dtype=ASSIGNMENT_DTYPE)
    out["fI"] = -1
    out["second_fi"] = -1
    out["otu"] = -1
    return out


def _otu_of(otu, n):
    if otu is None:
        return np.full(n, -1, np.int32)
    o = np.asarray(otu, dtype=OTU_DTYPE)
    return np.where(o["n"] > 0, o["oI"][:, 0], -1).astype(np.int32)


def assign(calls, call_start, otu=None, min_score: int = 0, min_share_pct: int = 50) -> np.ndarray:
    """calls CALL_DTYPE, call_start int64[n + 1] (non-decreasing), otu OTU_DTYPE[n] or None -> ASSIGNMENT_DTYPE[n]."""
    cs = np.asarray(call_start, dtype=np.int64)
    n = cs.size - 1
    out = _empty(n)
    if n <= 0:
        return out
    out["otu"] = _otu_of(otu, n)
    cnt = cs[1:] - cs[:-1]
    assert (cnt >= 0).all()
    c = np.asarray(calls, dtype=CALL_DTYPE)[cs[0]:cs[-1]]
    out["n_calls"] = cnt
    if c.size == 0:
        return out
    prot = np.repeat(np.arange(n, dtype=np.int64), cnt)
    f = c["fI"].astype(np.int64)
    order = np.lexsort((f, prot))                   # stable: emission order inside one (protein, function)
    ps, fs = prot[order], f[order]
    ks = c["count"].astype(np.int64)[order]
    ws = c["weightedHits"].astype(np.float32)[order]
    m = ps.size
    head = np.ones(m, dtype=bool)
    head[1:] = (ps[1:] != ps[:-1]) | (fs[1:] != fs[:-1])
    first = np.flatnonzero(head)
    rid = np.cumsum(head) - 1
    S = np.add.reduceat(ks, first)
    # W_f: float32 adds in emission order, the j-th CALL of every run at step j
    pos = np.arange(m) - first[rid]
    W = np.zeros(first.size, dtype=np.float32)
    by_pos = np.argsort(pos, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(pos))])
    for j in range(bounds.size - 1):
        idx = by_pos[bounds[j]:bounds[j + 1]]
        r = rid[idx]
        W[r] = W[r] + ws[idx]
    rp, rf = ps[first], fs[first]
    rank = np.lexsort((rf, -W, -S, rp))             # per protein: S desc, W desc, f asc
    rp, rf, S, W = rp[rank], rf[rank], S[rank], W[rank]
    pfirst = np.flatnonzero(np.concatenate([[True], rp[1:] != rp[:-1]]))
    nf = np.diff(np.concatenate([pfirst, [rp.size]]))
    P = rp[pfirst]
    T = np.add.reduceat(S, pfirst)
    out["fI"][P] = rf[pfirst]
    out["score"][P] = S[pfirst]
    out["weighted"][P] = W[pfirst]
    out["total"][P] = T
    out["n_functions"][P] = nf
    two = nf > 1
    out["second_fi"][P[two]] = rf[pfirst[two] + 1]
    out["second_score"][P[two]] = S[pfirst[two] + 1]
    Sb = S[pfirst]
    out["assigned"][P] = ((Sb >= min_score) & (100 * Sb >= np.int64(min_share_pct) * T)).astype(np.int32)
    return out


def brute_force(calls, call_start, otu=None, min_score: int = 0, min_share_pct: int = 50) -> np.ndarray:
    """The same rule, one protein at a time with a dict."""
    cs = [int(x) for x in call_start]
    n = len(cs) - 1
    out = _empty(max(n, 0))
    oo = _otu_of(otu, max(n, 0))
    for p in range(n):
        grp = {}
        total = 0
        for r in calls[cs[p]:cs[p + 1]]:
            f, k, w = int(r["fI"]), int(r["count"]), np.float32(r["weightedHits"])
            s, acc = grp.get(f, (0, np.float32(0)))
            grp[f] = (s + k, np.float32(acc + w))
            total += k
        ranked = sorted(grp.items(), key=lambda kv: (-kv[1][0], -float(kv[1][1]), kv[0]))
        rec = out[p]
        rec["n_calls"] = cs[p + 1] - cs[p]
        rec["otu"] = oo[p]
        if ranked:
            (fb, (sb, wb)) = ranked[0]
            rec["fI"], rec["score"], rec["weighted"], rec["total"] = fb, sb, wb, total
            rec["n_functions"] = len(ranked)
            rec["assigned"] = int(sb >= min_score and 100 * sb >= min_share_pct * total)
            if len(ranked) > 1:
                rec["second_fi"], rec["second_score"] = ranked[1][0], ranked[1][1][0]
        out[p] = rec
    return out


def random_lists(rng, n_prot: int, max_calls: int = 6, n_fn: int = 4, max_count: int = 6):
    """Random CALL lists with many ties: small function sets, small counts, weights from a few values."""
    cnt = rng.integers(0, max_calls + 1, size=n_prot)
    cs = np.zeros(n_prot + 1, dtype=np.int64)
    cs[1:] = np.cumsum(cnt)
    m = int(cs[-1])
    calls = np.zeros(m, dtype=CALL_DTYPE)
    calls["container"] = np.repeat(np.arange(n_prot, dtype=np.uint32), cnt)
    calls["fI"] = rng.integers(0, n_fn, size=m)
    calls["count"] = rng.integers(2, max_count + 1, size=m)
    calls["weightedHits"] = rng.choice(np.array([0.5, 1.0, 1.25, 2.0, 3.0, 0.1], np.float32), size=m)
    otu = np.zeros(n_prot, dtype=OTU_DTYPE)
    otu["n"] = rng.integers(0, 3, size=n_prot)
    otu["oI"][:, 0] = rng.integers(0, 9, size=n_prot)
    otu["count"][:, 0] = 1
    return calls, cs, otu
