"""The ops of a traced alignment (include/kmerguts_hip.h, "the alignments themselves") restated on top of tests/trace_model.py: the
walk's column string, reversed into alignment order and run-length encoded in both modes, and ops_model, which does that for a
batch of pairs the way paths_model makes their path records.  The GPU tests compare the device's bytes with this."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import GAP_EXTEND, GAP_OPEN

import align_model as A
import trace_model as T

MODES = ("m", "eqx")


def kinds_of(a: bytes, b: bytes, rec, cols: str, mode: str) -> str:
    """The kind of every column, in alignment order: cols is walk()'s string (end to start: 'M' a residue pair, 'E' (-, b_j),
    'F' (a_i, -)), rec the path record that gives the start."""
    ca, cb = A.codes(a), A.codes(b)
    i, j = rec[0], rec[1]
    out = []
    for c in reversed(cols):
        if c == "M":
            same = ca[i] == cb[j] and ca[i] < 20
            out.append("M" if mode == "m" else "=" if same else "X")
            i += 1
            j += 1
        elif c == "F":                                  # (a_i, -): consumes the query only
            out.append("I")
            i += 1
        else:                                           # (-, b_j): consumes the target only
            out.append("D")
            j += 1
    return "".join(out)


CODES = {"M": N.OP_M, "I": N.OP_I, "D": N.OP_D, "=": N.OP_EQ, "X": N.OP_X}


def encode(kinds: str) -> list:
    """Maximal runs of one kind -> len << 4 | code."""
    ops, k = [], 0
    while k < len(kinds):
        e = k
        while e < len(kinds) and kinds[e] == kinds[k]:
            e += 1
        ops.append((e - k) << 4 | CODES[kinds[k]])
        k = e
    return ops


_TRACED = {}                                # the walks of this process, shared by the two modes: a trace is the expensive part


def _traced(a, b, S, gap_open, gap_extend, end, trace):
    key = (bytes(a), bytes(b), np.asarray(S, dtype=np.int64).tobytes(), int(gap_open), int(gap_extend), end, trace)
    if key not in _TRACED:
        if len(_TRACED) > 4096:
            _TRACED.clear()
        _TRACED[key] = trace(a, b, S, gap_open, gap_extend, end=end, with_columns=True)
    return _TRACED[key]


def ops_of(a: bytes, b: bytes, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, mode: str = "m", end=None,
           trace=T.trace_numpy):
    """-> (end, the path's seven fields or None, the ops as a list)."""
    end, rec, cols = _traced(a, b, S, gap_open, gap_extend, end, trace)
    if rec is None:
        return end, None, []
    return end, rec, encode(kinds_of(a[:end[1] + 1], b[:end[2] + 1], rec, cols, mode))


def ops_model(seq: bytes, offsets, pairs, aln, mode: str, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
              max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, want=None):
    """As trace_model.paths_model, with the ops: -> (ALIGN_PATH_DTYPE records, op_start int64[n + 1], ops uint32)."""
    seq = bytes(seq)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=N.ALIGN_PATH_DTYPE)
    starts, ops, memo = [0], [], {}
    for k, (a, b) in enumerate(pairs):
        score, ea, eb = int(aln["score"][k]), int(aln["end_a"][k]), int(aln["end_b"][k])
        asked = int(aln["status"][k]) == 0 if want is None else bool(want[k])
        if not asked or score <= 0:
            out[k] = T.NO_PATH + (N.PATH_NONE,)
        elif (ea + 1) * (eb + 1) > max_trace_cells:
            out[k] = T.NO_PATH + (N.PATH_UNTRACED,)
        else:
            pa, pb = seq[offsets[a]:offsets[a + 1]], seq[offsets[b]:offsets[b + 1]]
            key = (pa, pb, score, ea, eb)
            if key not in memo:
                memo[key] = ops_of(pa, pb, S, gap_open, gap_extend, mode, end=(score, ea, eb))[1:]
            out[k] = memo[key][0] + (N.PATH_TRACED,)
            ops += memo[key][1]
        starts.append(len(ops))
    return out, np.asarray(starts, dtype=np.int64), np.asarray(ops, dtype=np.uint32)


def search_ops_model(seq: bytes, offsets, n_db: int, mode: str, paths: str = "hits", max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS,
                     searched=None, **kw):
    """trace_model.search_paths_model with the ops: -> (hits, hit_start, path records, op_start, ops)."""
    import search_model as SM
    hits, start, _ = searched if searched is not None else SM.search_model(seq, offsets, n_db, **kw)
    S = A.S62 if kw.get("matrix") is None else np.asarray(kw["matrix"], dtype=np.int64)
    want = hits["status"] == N.SEARCH_HIT if paths == "hits" else (hits["status"] != N.SEARCH_SKIPPED) & (hits["score"] >= 1)
    aln = {"score": hits["score"], "end_a": hits["end_query"], "end_b": hits["end_target"], "status": hits["status"]}
    pairs = np.stack([hits["query"].astype(np.int64) + n_db, hits["target"].astype(np.int64)], axis=1) if len(hits) else np.zeros((0, 2))
    recs, op_start, ops = ops_model(seq, offsets, pairs, aln, mode, S, kw.get("gap_open", GAP_OPEN), kw.get("gap_extend", GAP_EXTEND),
                                    max_trace_cells, want)
    return hits, start, recs, op_start, ops


def merged(ops) -> list:
    """'=' and 'X' ops as M, neighbours joined: what the eqx ops must give in M mode."""
    out = []
    for x in ops:
        ln, code = int(x) >> 4, int(x) & 15
        code = N.OP_M if code in (N.OP_EQ, N.OP_X) else code
        if out and out[-1] & 15 == code:
            out[-1] += ln << 4
        else:
            out.append(ln << 4 | code)
    return out


def check_invariants(end, rec, ops_m, ops_x):
    """The header's statements about a traced record's ops."""
    def total(ops, code):
        return sum(int(x) >> 4 for x in ops if int(x) & 15 == code)
    ra, rb, columns = T.columns_of(end, rec)
    assert len(ops_m) <= 2 * rec[4] + 1
    assert total(ops_m, N.OP_I) == rec[6] and total(ops_m, N.OP_D) == rec[5] and total(ops_m, N.OP_M) == ra == rb
    assert total(ops_x, N.OP_EQ) == rec[2] and merged(ops_x) == list(ops_m)
    assert sum(int(x) >> 4 for x in ops_m) == columns == sum(int(x) >> 4 for x in ops_x)
    assert all(int(x) >> 4 >= 1 for x in list(ops_m) + list(ops_x))
