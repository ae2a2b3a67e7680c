"""numpy / plain-Python model of the gene-set selection (include/kmerguts_hip.h, kg_regionset_select): `select` is the rule as
written -- sort by strength, loop, test against the selected so far; `brute_force` tries all pairs and iterates to the fixed
point; plus the generators the host and GPU tests share."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd._native import INTERVAL_DTYPE, SELECTION_DTYPE


def intervals(rows) -> np.ndarray:
    """rows of (seq, left, right, score[, eligible]) -> INTERVAL_DTYPE."""
    out = np.zeros(len(rows), dtype=INTERVAL_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(r) + ((1,) if len(r) == 4 else ())
    return out


def of_records(recs) -> np.ndarray:
    """The candidates of region or ORF records: their extent, score and kept."""
    out = np.zeros(len(recs), dtype=INTERVAL_DTYPE)
    for name, src in (("seq", "seq"), ("left", "left"), ("right", "right"), ("score", "score"), ("eligible", "kept")):
        out[name] = recs[src]
    return out


def conflict(a, b, max_overlap: int, pct: int) -> bool:
    """rule 2 for two eligible candidates (Python ints: no overflow)."""
    if int(a["seq"]) != int(b["seq"]):
        return False
    ov = min(int(a["right"]), int(b["right"])) - max(int(a["left"]), int(b["left"])) + 1
    if ov <= 0:
        return False
    shorter = min(int(a["right"]) - int(a["left"]) + 1, int(b["right"]) - int(b["left"]) + 1)
    return ov > max_overlap or 100 * ov > pct * shorter


def strength_order(iv) -> list:
    """rule 3: the eligible candidates' indices, strongest first."""
    idx = [i for i in range(len(iv)) if iv["eligible"][i]]
    return sorted(idx, key=lambda i: (-int(iv["score"][i]), -(int(iv["right"][i]) - int(iv["left"][i]) + 1), i))


def select(iv, max_overlap: int = 60, pct: int = 50):
    """-> (SELECTION_DTYPE[n], stats dict of the counts kg_select_stats has).  The literal rule; the selected so far are kept
    per contig and sorted by nothing: every one is tested."""
    iv = np.asarray(iv, dtype=INTERVAL_DTYPE)
    out = np.zeros(len(iv), dtype=SELECTION_DTYPE)
    out["by"] = -1
    chosen = {}
    for i in strength_order(iv):
        beaten = [j for j in chosen.get(int(iv["seq"][i]), []) if conflict(iv[i], iv[j], max_overlap, pct)]
        if beaten:
            out[i] = (2, min(beaten))
        else:
            out[i] = (1, -1)
            chosen.setdefault(int(iv["seq"][i]), []).append(i)
    return out, stats(iv, out, max_overlap, pct)


def stats(iv, out, max_overlap: int, pct: int) -> dict:
    """candidates, eligible, selected, overlapped, pairs (eligible, one contig, ov > 0) and conflicts, by a sweep per contig."""
    el = np.flatnonzero(iv["eligible"] != 0)
    pairs = conflicts = 0
    for s in np.unique(iv["seq"][el]):
        mine = el[iv["seq"][el] == s]
        mine = mine[np.argsort(iv["left"][mine], kind="stable")]
        left, right = iv["left"][mine].astype(np.int64), iv["right"][mine].astype(np.int64)
        for a in range(len(mine)):
            b_end = int(np.searchsorted(left, right[a], side="right"))
            for b in range(a + 1, b_end):
                pairs += 1
                conflicts += bool(conflict(iv[mine[a]], iv[mine[b]], max_overlap, pct))
    return {"candidates": len(iv), "eligible": len(el), "selected": int((out["state"] == 1).sum()),
            "overlapped": int((out["state"] == 2).sum()), "pairs": pairs, "conflicts": conflicts}


def select_fast(iv, max_overlap: int = 60, pct: int = 50):
    """`select` for large lists: the same loop, the selected of a contig kept sorted by left with a running maximum of right,
    so that only those that can overlap are tested.  -> SELECTION_DTYPE[n] (no stats)."""
    import bisect
    iv = np.asarray(iv, dtype=INTERVAL_DTYPE)
    out = np.zeros(len(iv), dtype=SELECTION_DTYPE)
    out["by"] = -1
    el = np.flatnonzero(iv["eligible"] != 0)
    length = iv["right"].astype(np.int64) - iv["left"] + 1
    order = el[np.lexsort((el, -length[el], -iv["score"][el].astype(np.int64)))]
    chosen = {}
    # selected intervals that do not conflict may still overlap a little, so a candidate looks at every selected one whose left
    # is within the longest selected length of its own
    for i in order.tolist():
        s, l, r = int(iv["seq"][i]), int(iv["left"][i]), int(iv["right"][i])
        lefts, ids, longest = chosen.setdefault(s, ([], [], [0]))
        lo = bisect.bisect_left(lefts, l - longest[0])
        hi = bisect.bisect_right(lefts, r)
        beaten = [j for j in ids[lo:hi] if conflict(iv[i], iv[j], max_overlap, pct)]
        if beaten:
            out[i] = (2, min(beaten))
        else:
            out[i] = (1, -1)
            at = bisect.bisect_right(lefts, l)
            lefts.insert(at, l)
            ids.insert(at, i)
            longest[0] = max(longest[0], r - l + 1)
    return out


def brute_force(iv, max_overlap: int = 60, pct: int = 50) -> np.ndarray:
    """All pairs, then sweeps to the fixed point: an undecided candidate all of whose stronger conflicting candidates are
    overlapped becomes selected, one with a selected stronger conflicting candidate becomes overlapped."""
    iv = np.asarray(iv, dtype=INTERVAL_DTYPE)
    n = len(iv)
    rank = {i: k for k, i in enumerate(strength_order(iv))}
    stronger = {i: [] for i in rank}
    for i in rank:
        for j in rank:
            if rank[j] < rank[i] and conflict(iv[i], iv[j], max_overlap, pct):
                stronger[i].append(j)
    state = {i: 0 for i in rank}
    changed = True
    while changed:
        changed = False
        for i in rank:
            if state[i]:
                continue
            if any(state[j] == 1 for j in stronger[i]):
                state[i], changed = 2, True
            elif all(state[j] == 2 for j in stronger[i]):
                state[i], changed = 1, True
    out = np.zeros(n, dtype=SELECTION_DTYPE)
    out["by"] = -1
    for i in rank:
        assert state[i] in (1, 2)
        out[i] = (state[i], min(j for j in stronger[i] if state[j] == 1) if state[i] == 2 else -1)
    return out


def check_properties(iv, out, max_overlap: int, pct: int) -> None:
    """No two selected conflict; every overlapped one has a stronger selected conflicting candidate at `by`; no overlapped one
    could be added; non-eligible records are (0, -1)."""
    iv = np.asarray(iv, dtype=INTERVAL_DTYPE)
    rank = {i: k for k, i in enumerate(strength_order(iv))}
    sel = [i for i in rank if out["state"][i] == 1]
    for i in range(len(iv)):
        if i not in rank:
            assert tuple(out[i]) == (0, -1)
    for a in sel:
        assert out["by"][a] == -1
        for b in sel:
            assert a == b or not conflict(iv[a], iv[b], max_overlap, pct), (a, b)
    for i in rank:
        if out["state"][i] == 2:
            by = int(out["by"][i])
            assert out["state"][by] == 1 and rank[by] < rank[i] and conflict(iv[i], iv[by], max_overlap, pct), i
            assert any(conflict(iv[i], iv[j], max_overlap, pct) for j in sel), i
        else:
            assert out["state"][i] == 1


# ---- generators ----

def random_list(rng, n: int, n_seqs: int = 3, span: int = 2000, max_len: int = 300, max_score: int = 40, p_eligible: float = 0.85):
    iv = np.zeros(n, dtype=INTERVAL_DTYPE)
    iv["seq"] = rng.integers(0, n_seqs, n)
    iv["left"] = rng.integers(0, span, n)
    iv["right"] = iv["left"] + rng.integers(0, max_len, n)
    iv["score"] = rng.integers(0, max_score, n)
    iv["eligible"] = rng.random(n) < p_eligible
    return iv


def nested(n: int, seq: int = 0, step: int = 3, score_up: bool = True):
    """n intervals, each inside the one in front."""
    return intervals([(seq, step * k, 2 * step * n - step * k, (k if score_up else n - k)) for k in range(n)])


def staircase(n: int, seq: int = 0, step: int = 10, length: int = 16, descending: bool = True):
    """Each step conflicts with the next one only (length 16, shifted by 10: ov 6 of 16 is over 0 %); with descending scores the
    decisions wait for each other along the whole chain."""
    return intervals([(seq, step * k, step * k + length - 1, (n - k if descending else k)) for k in range(n)])


def identical(n: int, seq: int = 0, left: int = 100, right: int = 400, score: int = 7):
    return intervals([(seq, left, right, score)] * n)


def shuffled(rng, iv):
    """The list in another order and the permutation: shuffled[k] = iv[perm[k]]."""
    perm = rng.permutation(len(iv))
    return iv[perm].copy(), perm
