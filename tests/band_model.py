"""The band rule of kg_proteins_align_banded / kg_proteins_search_banded (include/kmerguts_hip.h) restated: align_model's
recurrence with the cells outside the band forced to H = 0, as plain loops and by anti-diagonals with numpy; the banded walk,
which is trace_model's walk over such tables; and the banded search, ungapped_model's candidates aligned in the band around their
g*.  The GPU tests compare the device's bytes with the numpy form; the CPU tests compare the two forms with each other, with
align_model and ungapped_model at the band's two ends, and with answers worked out by hand."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import GAP_EXTEND, GAP_OPEN, MIN_RATIO_PCT

import align_model as A
import ops_model as O
import search_model as SM
import seed_model as SD
import trace_model as T
import ungapped_model as U

BAND_MAX = 256
NEG = T.NEG


def in_band(i: int, j: int, g: int, W: int) -> bool:
    """0-based (i, j): a_i against b_j."""
    return abs((i - j) - g) <= W


def band_cells(n: int, m: int, W: int) -> int:
    """What counts against max_cells."""
    return min(n * m, min(n, m) * (2 * W + 1))


def covering(n: int, m: int, g: int) -> int:
    """The smallest W >= 0 whose band around g holds every cell of an n x m matrix."""
    return max(n - 1 - g, m - 1 + g, 0)


# ---- the tables: H, E, F, 1-based with the boundary row and column, out-of-band cells with H = 0 ----------------------------------

def tables_loops(ca, cb, g, W, S, gap_open, gap_extend):
    n, m = len(ca), len(cb)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(E[i][j - 1], H[i][j - 1] - gap_open) - gap_extend
            F[i][j] = max(F[i - 1][j], H[i - 1][j] - gap_open) - gap_extend
            if in_band(i - 1, j - 1, g, W):
                H[i][j] = max(0, H[i - 1][j - 1] + int(S[ca[i - 1]][cb[j - 1]]), E[i][j], F[i][j])
    return H, E, F


def tables_numpy(ca, cb, g, W, S, gap_open, gap_extend):
    """The same by anti-diagonals d = i + j."""
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
        h = np.maximum(np.maximum(0, H[i - 1, j - 1] + S[ca[i - 1], cb[j - 1]]), np.maximum(e, f))
        H[i, j] = np.where(np.abs((i - j) - g) <= W, h, 0)
    return H, E, F


def _caps(gap_open, gap_extend):
    return min(int(gap_open), T.GAP_CAP), min(int(gap_extend), T.GAP_CAP)


def _end(H, n, m):
    """(score, end_a, end_b): the first maximum row by row, left to right; an out-of-band cell has H = 0 and never is one."""
    if n == 0 or m == 0:
        return (0, -1, -1)
    body = np.asarray(H, dtype=np.int64)[1:, 1:]
    k = int(np.argmax(body))
    top = int(body.flat[k])
    return (top, k // m, k % m) if top > 0 else (0, -1, -1)


def band_loops(a: bytes, b: bytes, g: int, W: int, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND):
    """-> (score, end_a, end_b) under the band (g, W), one cell at a time."""
    go, ge = _caps(gap_open, gap_extend)
    ca, cb = T._codes(a), T._codes(b)
    H, _, _ = tables_loops(ca, cb, g, W, S, go, ge)
    return T.end_cell(H, len(ca), len(cb))


def band_numpy(a: bytes, b: bytes, g: int, W: int, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND):
    go, ge = _caps(gap_open, gap_extend)
    ca, cb = T._codes(a), T._codes(b)
    H, _, _ = tables_numpy(ca, cb, g, W, S, go, ge)
    return _end(H, len(ca), len(cb))


def band_trace(a: bytes, b: bytes, g: int, W: int, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, end=None,
               tables=tables_numpy):
    """-> ((score, end_a, end_b), the path's seven fields or None, the walk's column string).  The walk is trace_model.walk over
    the prefix box's tables with the out-of-band cells forced to H = 0."""
    go, ge = _caps(gap_open, gap_extend)
    ca, cb = T._codes(a), T._codes(b)
    if end is None:
        H, _, _ = tables(ca, cb, g, W, S, go, ge)
        end = _end(H, len(ca), len(cb))
    if end[0] <= 0:
        return end, None, ""
    ca, cb = ca[:end[1] + 1], cb[:end[2] + 1]
    H, E, F = tables(ca, cb, g, W, S, go, ge)
    assert int(H[end[1] + 1][end[2] + 1]) == end[0], "the box's end cell does not reproduce the score"
    rec, cols = T.walk(H, E, F, ca, cb, S, go, ge, end[1], end[2])
    return end, rec, cols


# ---- batches ---------------------------------------------------------------------------------------------------------------------

def align_model(seq: bytes, offsets, pairs, diagonals, W: int, S=A.S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
                max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, sw=band_numpy) -> np.ndarray:
    """-> ALIGNMENT_DTYPE records in pair order."""
    seq = bytes(seq)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=N.ALIGNMENT_DTYPE)
    memo = {}
    for k, (a, b) in enumerate(pairs):
        pa, pb = seq[offsets[a]:offsets[a + 1]], seq[offsets[b]:offsets[b + 1]]
        g = int(diagonals[k])
        if band_cells(len(pa), len(pb), W) > max_cells:
            r = (-1, -1, -1, N.ALIGN_SKIPPED)
        else:
            if (pa, pb, g) not in memo:
                memo[(pa, pb, g)] = sw(pa, pb, g, W, S, gap_open, gap_extend)
            r = memo[(pa, pb, g)] + (N.ALIGN_ALIGNED,)
        out[k] = (r[0], A.self_score(pa, S), A.self_score(pb, S), r[1], r[2], r[3])
    return out


def ops_model(seq: bytes, offsets, pairs, diagonals, W: int, aln, mode: str = "m", S=A.S62, gap_open: int = GAP_OPEN,
              gap_extend: int = GAP_EXTEND, max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, want=None):
    """ops_model.ops_model under the band: -> (ALIGN_PATH_DTYPE records, op_start int64[n + 1], ops uint32)."""
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
            key = (pa, pb, int(diagonals[k]), score, ea, eb)
            if key not in memo:
                _, rec, cols = band_trace(pa, pb, int(diagonals[k]), W, S, gap_open, gap_extend, end=(score, ea, eb))
                memo[key] = (rec, O.encode(O.kinds_of(pa[:ea + 1], pb[:eb + 1], rec, cols, mode)))
            out[k] = memo[key][0] + (N.PATH_TRACED,)
            ops += memo[key][1]
        starts.append(len(ops))
    return out, np.asarray(starts, dtype=np.int64), np.asarray(ops, dtype=np.uint32)


def search_model(seq: bytes, offsets, n_db: int, W: int, seed=None, seeding=None, min_ungapped: int = 0, min_shared: int = SM.MIN_SHARED,
                 max_cand: int = SM.MAX_CAND, max_db_per_kmer: int = SM.MAX_DB_PER_KMER, matrix=None, min_ratio_pct: int = MIN_RATIO_PCT,
                 ref="longer", gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS):
    """ungapped_model.filtered_model with every kept candidate aligned in the band (g*, W): -> (SEARCH_HIT_DTYPE records in (query,
    rank) order, hit_start, SEARCH_UNGAPPED_DTYPE records of the same indices, the counts of kg_search_stats, of
    kg_ungapped_stats and of kg_band_stats)."""
    seq = bytes(seq)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_q = len(offsets) - 1 - n_db
    S = A.S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    ref = N.ALIGN_REFS.get("member" if ref == "query" else ref, ref)
    seed_set = SD.EXACT if seed is None else seed
    cands = U.scored(seq, offsets, n_db, seed, seeding, min_shared, max_db_per_kmer, matrix)
    kept, dropped, n_cut = U.cut(cands, n_q, min_ungapped, max_cand)
    _, counts = SD.shared_numpy(seed_set)(seq if seeding is None else seeding, offsets, n_db, max_db_per_kmer)
    counts["candidates"] = len(cands)
    pairs = [(n_db + q, c[0]) for q in range(n_q) for c in kept[q]]
    diag = [c[2] for q in range(n_q) for c in kept[q]]
    aln = align_model(seq, offsets, pairs, diag, W, S, gap_open, gap_extend, max_cells)
    hits = np.zeros(len(pairs), dtype=N.SEARCH_HIT_DTYPE)
    ung = np.zeros(len(pairs), dtype=N.SEARCH_UNGAPPED_DTYPE)
    start = np.zeros(n_q + 1, dtype=np.int64)
    counts.update(aligned=0, hits=0, skipped=0, queries_hit=0, cells=0)
    band = dict(band_cells=0, full_cells=0, band=W)
    k = 0
    for q in range(n_q):
        recs = []
        for d, s, g, m, u in kept[q]:
            a = aln[k]
            k += 1
            r = int(a["self_a"]) if ref == N.ALIGN_REF_MEMBER else max(int(a["self_a"]), int(a["self_b"]))
            nq, nd = int(offsets[n_db + q + 1] - offsets[n_db + q]), int(offsets[d + 1] - offsets[d])
            if a["status"] == N.ALIGN_SKIPPED:
                status = N.SEARCH_SKIPPED
                counts["skipped"] += 1
            else:
                status = N.SEARCH_HIT if A.kept(int(a["score"]), r, min_ratio_pct) else N.SEARCH_BELOW
                counts["aligned"] += 1
                counts["hits"] += status == N.SEARCH_HIT
                counts["cells"] += nq * nd
                band["band_cells"] += band_cells(nq, nd, W)
                band["full_cells"] += nq * nd
            recs.append((q, d, s, int(a["score"]), int(a["self_a"]), int(a["self_b"]), int(a["end_a"]), int(a["end_b"]), status, (u, g, m, 0)))
        recs.sort(key=lambda x: (x[8] == N.SEARCH_SKIPPED, -x[3], -x[2], x[1]))
        for rank, x in enumerate(recs):
            hits[start[q] + rank] = x[:9] + (rank,)
            ung[start[q] + rank] = x[9]
        start[q + 1] = start[q] + len(recs)
        counts["queries_hit"] += bool(recs) and recs[0][8] == N.SEARCH_HIT
    counts = {key: int(v) for key, v in counts.items()}
    return hits, start, ung, counts, dict(scored=len(cands), dropped=dropped, cut=n_cut, cells=sum(
        U.cells_of(int(offsets[n_db + q + 1] - offsets[n_db + q]), int(offsets[d + 1] - offsets[d]), g)
        for (q, d), (s, g, m, u) in cands.items())), band


def search_ops_model(seq: bytes, offsets, n_db: int, W: int, hits, ung, mode: str = "m", paths: str = "hits",
                     max_trace_cells: int = N.TRACE_DEFAULT_MAX_CELLS, matrix=None, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND):
    """The banded trace behind search_model's records: -> (path records, op_start, ops)."""
    S = A.S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    want = hits["status"] == N.SEARCH_HIT if paths == "hits" else (hits["status"] != N.SEARCH_SKIPPED) & (hits["score"] >= 1)
    aln = {"score": hits["score"], "end_a": hits["end_query"], "end_b": hits["end_target"], "status": hits["status"]}
    pairs = np.stack([hits["query"].astype(np.int64) + n_db, hits["target"].astype(np.int64)], axis=1) if len(hits) else np.zeros((0, 2))
    return ops_model(seq, offsets, pairs, ung["diagonal"], W, aln, mode, S, gap_open, gap_extend, max_trace_cells, want)


# ---- hand-made cases: their answers follow from how they are made ---------------------------------------------------------------

def blocks(rng, k: int, avoid: bytes = b"") -> bytes:
    """k random residues, none of `avoid`."""
    letters = bytes(ch for ch in A.ALPHA if ch not in avoid)
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), k))


SUFFIX = b"CPHDKITA"                 # eight distinct residues; with W and G every pair of two different ones scores <= 0 in BLOSUM62


def insert_case(k: int = 6, lp: int = 30, mirror: bool = False):
    """a = P + k inserted residues + S against b = P + S (mirror: the other way round), g = 0.  P is lp tryptophans (11 each), S
    is SUFFIX (self-score 48), the insert glycines: only identical residues score above 0, and S has no residue twice, so S scores
    on S at the shift k alone.  With a band of at least k the joined alignment P, gap, S is in the band and nothing beats it
    (17 < 48 for k = 6); below k no cell of S on S is, and the score is P's.  -> (a, b, joined score, P's score)"""
    P, ins = b"W" * lp, b"G" * k
    a, b = P + ins + SUFFIX, P + SUFFIX
    joined = 11 * lp + A.self_score(SUFFIX) - (GAP_OPEN + k * GAP_EXTEND)
    return (b, a, joined, 11 * lp) if mirror else (a, b, joined, 11 * lp)


def feature_case():
    """a = X + Y, b = X + 40 other residues + Y, g = 0: the full alignment joins X and Y across a 40-residue gap, the band of 8
    cannot.  X is 60 tryptophans (660), Y 30 cysteines (270), the filler glycines.  -> (a, b, X's score, the joined score)"""
    X, Y = b"W" * 60, b"C" * 30
    return X + Y, X + b"G" * 40 + Y, 11 * 60, 11 * 60 + 9 * 30 - (GAP_OPEN + 40 * GAP_EXTEND)


def with_indels(rng, p: bytes, every: int = 50, longest: int = 10) -> bytes:
    """p with an insertion of random residues or a deletion, of 1 to `longest` residues, about every `every`-th residue."""
    out, at = bytearray(), 0
    while at < len(p):
        step = int(rng.integers(every // 2, every + every // 2))
        out += p[at:at + step]
        at += step
        k = int(rng.integers(1, longest + 1))
        if at < len(p):
            if rng.random() < 0.5:
                out += bytes(A.ALPHA[int(x)] for x in rng.integers(0, 20, k))
            else:
                at += k
    return bytes(out)


def indel_search(seed: int, n_targets: int = 8, n_related: int = 5, length: int = 110, every: int = 35):
    """Random targets; queries that are 8 %-substituted copies of targets 0 .. n_related - 1 with indels of 1 to 10 residues, and
    two unrelated ones.  -> (proteins, n_db)"""
    rng = np.random.default_rng(seed)
    targets = [A.M.random_protein(rng, int(rng.integers(length - 30, length + 30))) for _ in range(n_targets)]
    related = [with_indels(rng, A.mutate(rng, targets[k], 0.08), every) for k in range(n_related)]
    return targets + related + [A.M.random_protein(rng, length) for _ in range(2)], n_targets


def tie_cases():
    """((a, b, g, W), (score, end_a, end_b)) by construction: one scoring cell each, no two of them on one diagonal run."""
    out = []
    a, b = b"WGGGGWGG", b"PPPPWPPP"       # W / W at (0, 4), i - j = -4, and at (5, 4), i - j = 1
    out.append(((a, b, 0, 1), (11, 5, 4)))                  # the cell with the smaller i is outside the band and must not win
    out.append(((a, b, 0, 4), (11, 0, 4)))                  # ... inside it, it does
    out.append(((a, b, -3, 1), (11, 0, 4)))
    out.append(((b"GYGPG", b"DPDYD", 0, 2), (7, 1, 3)))     # (1, 3) and (3, 1): the smaller i
    out.append(((b"GGYGG", b"DYDYD", 0, 2), (7, 2, 1)))     # (2, 1) and (2, 3): the smaller j
    out.append(((b"GGYGG", b"DYDYD", 0, 0), (0, -1, -1)))   # neither on the diagonal itself
    out.append(((b"GYGGG" + b"G" * 65 + b"PG", b"DDDYD" + b"D" * 65 + b"PD", 0, 2), (7, 1, 3)))        # (1, 3) and (70, 70): across a stripe
    return out
