"""The traceback rule of kg_proteins_align_paths / kg_proteins_search_paths (include/kmerguts_hip.h) restated: the walk over full
H, E and F tables filled by plain loops, one cell at a time; the same tables filled by anti-diagonals with numpy, followed by
the same walk; and paths_model, which turns alignment records into path records.  The GPU tests compare the device's bytes with
the numpy form; the CPU tests compare the two forms with each other and with answers worked out by hand."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import GAP_EXTEND, GAP_OPEN

import align_model as A

GAP_CAP = 1 << 29                   # the alignment kernel's cap of either gap cost: the rule's `open` and `ext` are the capped ones
NEG = -(1 << 40)
NO_PATH = (-1, -1, 0, 0, 0, 0, 0)


def tables_loops(ca, cb, S, gap_open, gap_extend):
    """H, E, F as lists of lists, 1-based, boundary row and column included."""
    n, m = len(ca), len(cb)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(E[i][j - 1], H[i][j - 1] - gap_open) - gap_extend
            F[i][j] = max(F[i - 1][j], H[i - 1][j] - gap_open) - gap_extend
            H[i][j] = max(0, H[i - 1][j - 1] + int(S[ca[i - 1]][cb[j - 1]]), E[i][j], F[i][j])
    return H, E, F


def tables_numpy(ca, cb, S, gap_open, gap_extend):
    """The same tables filled by anti-diagonals d = i + j: a diagonal's cells need only the two diagonals before it."""
    ca, cb = np.asarray(ca, dtype=np.int64), np.asarray(cb, dtype=np.int64)
    n, m = ca.size, cb.size
    S = np.asarray(S, dtype=np.int64)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    E = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        e = np.maximum(E[i, j - 1], H[i, j - 1] - gap_open) - gap_extend
        f = np.maximum(F[i - 1, j], H[i - 1, j] - gap_open) - gap_extend
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(np.maximum(0, H[i - 1, j - 1] + S[ca[i - 1], cb[j - 1]]), np.maximum(e, f))
    return H, E, F


def end_cell(H, n, m):
    """(score, end_a, end_b): the cell with H = score that has the smallest i, then the smallest j; 0-based, (-1, -1) for 0."""
    best = (0, -1, -1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if H[i][j] > best[0]:
                best = (int(H[i][j]), i - 1, j - 1)
    return best


def walk(H, E, F, ca, cb, S, gap_open, gap_extend, end_a, end_b, ties=None):
    """The rule, word for word.  -> (the record's first seven fields, the column string: 'M' a residue pair, 'E' (-, b_j),
    'F' (a_i, -), from the end of the alignment to its start).  ties: a dict that counts the ties the walk met, by kind."""
    def tie(kind):
        if ties is not None:
            ties[kind] = ties.get(kind, 0) + 1

    i, j, state = end_a + 1, end_b + 1, "H"
    cols = []
    identical = positive = 0
    start = None
    for _ in range(2 * (i + j) + 2):
        if state == "H":
            assert H[i][j] > 0
            d, e, f = int(H[i][j] == H[i - 1][j - 1] + int(S[ca[i - 1]][cb[j - 1]])), int(H[i][j] == E[i][j]), int(H[i][j] == F[i][j])
            if d + e + f > 1:
                tie("all three" if d + e + f == 3 else "diagonal = E" if d and e else "diagonal = F" if d else "E = F")
            if H[i][j] == H[i - 1][j - 1] + int(S[ca[i - 1]][cb[j - 1]]):
                cols.append("M")
                identical += ca[i - 1] == cb[j - 1] and ca[i - 1] < 20
                positive += int(S[ca[i - 1]][cb[j - 1]]) > 0
                if i - 1 == 0 or j - 1 == 0 or H[i - 1][j - 1] == 0:
                    start = (i - 1, j - 1)              # 0-based (i, j)
                    break
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = "E"
            else:
                assert H[i][j] == F[i][j]
                state = "F"
        elif state == "E":
            cols.append("E")
            if E[i][j] == H[i][j - 1] - gap_open - gap_extend and E[i][j] == E[i][j - 1] - gap_extend:
                tie("E open = extend")
            state = "H" if E[i][j] == H[i][j - 1] - gap_open - gap_extend else "E"
            j -= 1
            assert j >= 1 and (state == "E" or H[i][j] > 0)
        else:
            cols.append("F")
            if F[i][j] == H[i - 1][j] - gap_open - gap_extend and F[i][j] == F[i - 1][j] - gap_extend:
                tie("F open = extend")
            state = "H" if F[i][j] == H[i - 1][j] - gap_open - gap_extend else "F"
            i -= 1
            assert i >= 1 and (state == "F" or H[i][j] > 0)
    assert start is not None, "the walk did not end"
    assert len(cols) <= (end_a + 1) + (end_b + 1)       # the moves: every column lowers the row, the column or both
    s = "".join(cols)
    opens = sum(1 for k, c in enumerate(s) if c != "M" and (k == 0 or s[k - 1] != c))
    return (start[0], start[1], int(identical), int(positive), opens, s.count("E"), s.count("F")), s


def _codes(p):
    return [int(x) for x in A.codes(p)]


def trace_loops(a: bytes, b: bytes, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, end=None, with_columns: bool = False,
                ties=None):
    """-> ((score, end_a, end_b), the path's seven fields or None).  Plain loops; end as for trace_numpy."""
    return _trace(tables_loops, a, b, S, gap_open, gap_extend, end, with_columns, ties)


def trace_numpy(a: bytes, b: bytes, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, end=None, with_columns: bool = False,
                ties=None):
    """The same by anti-diagonals.  end: (score, end_a, end_b) when it is known; the tables are then the prefix box's, whose
    cells have the values they have in the whole matrix."""
    return _trace(tables_numpy, a, b, S, gap_open, gap_extend, end, with_columns, ties)


def _trace(tables, a, b, S, gap_open, gap_extend, end, with_columns, ties=None):
    go, ge = min(int(gap_open), GAP_CAP), min(int(gap_extend), GAP_CAP)
    ca, cb = _codes(a), _codes(b)
    if end is not None and end[0] > 0:
        ca, cb = ca[:end[1] + 1], cb[:end[2] + 1]
    H, E, F = tables(ca, cb, S, go, ge)
    if end is None:
        end = end_cell(H, len(ca), len(cb))
    if end[0] <= 0:
        return (end, None, "") if with_columns else (end, None)
    assert int(H[end[1] + 1][end[2] + 1]) == end[0], "the box's end cell does not reproduce the score"
    rec, cols = walk(H, E, F, ca, cb, S, go, ge, end[1], end[2], ties)
    return (end, rec, cols) if with_columns else (end, rec)


def paths_model(seq: bytes, offsets, pairs, aln, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
                max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, want=None, trace=trace_numpy) -> np.ndarray:
    """aln: records with score / end_a / end_b / status (ALIGNMENT_DTYPE, or any array with these names); want[k]: whether pair
    k asks for a path (None: every aligned pair).  -> ALIGN_PATH_DTYPE records in pair order."""
    seq = bytes(seq)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=N.ALIGN_PATH_DTYPE)
    memo = {}
    for k, (a, b) in enumerate(pairs):
        score, ea, eb = int(aln["score"][k]), int(aln["end_a"][k]), int(aln["end_b"][k])
        asked = int(aln["status"][k]) == 0 if want is None else bool(want[k])
        if not asked or score <= 0:
            out[k] = NO_PATH + (N.PATH_NONE,)
        elif (ea + 1) * (eb + 1) > max_trace_cells:
            out[k] = NO_PATH + (N.PATH_UNTRACED,)
        else:
            pa, pb = seq[offsets[a]:offsets[a + 1]], seq[offsets[b]:offsets[b + 1]]
            key = (pa, pb, score, ea, eb)
            if key not in memo:
                memo[key] = trace(pa, pb, S, gap_open, gap_extend, end=(score, ea, eb))[1]
            out[k] = memo[key] + (N.PATH_TRACED,)
    return out


def columns_of(end, rec):
    """(residue columns by a, residue columns by b, columns) of a traced record: the header's formulas."""
    ra = (end[1] - rec[0] + 1) - rec[6]
    rb = (end[2] - rec[1] + 1) - rec[5]
    return ra, rb, ra + rec[5] + rec[6]


def search_paths_model(seq: bytes, offsets, n_db: int, paths: str = "hits", max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS,
                       trace=trace_numpy, searched=None, **kw):
    """search_model.search_model with the traceback behind it: -> (hit records, hit_start, one ALIGN_PATH_DTYPE record per hit
    record, the counts with traced / untraced / trace_cells).  paths "hits": the records with status hit are traced; "all":
    every aligned record with score >= 1.  a is the query, b the target.  searched: search_model's result, when the caller has it."""
    import search_model as SM
    hits, start, counts = searched if searched is not None else SM.search_model(seq, offsets, n_db, **kw)
    S = A.S62 if kw.get("matrix") is None else np.asarray(kw["matrix"], dtype=np.int64)
    want = hits["status"] == N.SEARCH_HIT if paths == "hits" else (hits["status"] != N.SEARCH_SKIPPED) & (hits["score"] >= 1)
    aln = {"score": hits["score"], "end_a": hits["end_query"], "end_b": hits["end_target"], "status": hits["status"]}
    pairs = np.stack([hits["query"].astype(np.int64) + n_db, hits["target"].astype(np.int64)], axis=1) if len(hits) else np.zeros((0, 2))
    recs = paths_model(seq, offsets, pairs, aln, S, kw.get("gap_open", GAP_OPEN), kw.get("gap_extend", GAP_EXTEND), max_trace_cells, want, trace)
    traced = recs["status"] == N.PATH_TRACED
    counts = dict(counts, traced=int(traced.sum()), untraced=int((recs["status"] == N.PATH_UNTRACED).sum()),
                  trace_cells=int(((hits["end_query"].astype(np.int64) + 1) * (hits["end_target"].astype(np.int64) + 1))[traced].sum()))
    return hits, start, recs, counts
