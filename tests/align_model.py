"""The alignment rule of kg_proteins_align / kg_proteins_cluster_aligned (include/kmerguts_hip.h) restated: the recurrence as
plain loops, one cell at a time; the same by anti-diagonals with numpy; and cluster_aligned_model, the family rule of
cluster_model.cluster_loops with the cut between the edge test and the components.  The GPU tests compare the device's bytes
with the numpy form; the CPU tests compare the two forms with each other and with answers worked out by hand."""
from __future__ import annotations

import numpy as np

from kmergutsjava_amd import _native as N
from kmergutsjava_amd.align_scores import ALPHA, BLOSUM62, GAP_EXTEND, GAP_OPEN, MIN_RATIO_PCT

import cluster_model as M

NEG = -(1 << 40)
S62 = np.array(BLOSUM62, dtype=np.int64)
_LUT = np.full(256, 20, dtype=np.int64)
_LUT[np.frombuffer(ALPHA, dtype=np.uint8)] = np.arange(20)


def codes(p: bytes) -> np.ndarray:
    return _LUT[np.frombuffer(bytes(p), dtype=np.uint8)]


def self_score(p: bytes, S=S62) -> int:
    c = codes(p)
    c = c[c < 20]
    return int(np.asarray(S)[c, c].sum())


def sw_loops(a: bytes, b: bytes, S=S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND):
    """The recurrence as written in the header.  -> (score, end_a, end_b), 0-based, (-1, -1) when the score is 0."""
    ca, cb = [int(x) for x in codes(a)], [int(x) for x in codes(b)]
    n, m = len(ca), len(cb)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    best = (0, -1, -1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(E[i][j - 1], H[i][j - 1] - gap_open) - gap_extend
            F[i][j] = max(F[i - 1][j], H[i - 1][j] - gap_open) - gap_extend
            H[i][j] = max(0, H[i - 1][j - 1] + int(S[ca[i - 1]][cb[j - 1]]), E[i][j], F[i][j])
            if H[i][j] > best[0]:                       # row by row, left to right: the first cell is the smallest i, then j
                best = (H[i][j], i - 1, j - 1)
    return best


def sw_numpy(a: bytes, b: bytes, S=S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND):
    """The same by anti-diagonals d = i + j: a diagonal's cells need only the two diagonals before it.  Arrays are indexed by
    the 1-based row i; entry 0 is the boundary row."""
    ca, cb = codes(a), codes(b)
    n, m = ca.size, cb.size
    if n == 0 or m == 0:
        return (0, -1, -1)
    S = np.asarray(S, dtype=np.int64)
    H1 = np.zeros(n + 1, dtype=np.int64)                # diagonal d - 1, by row
    H2 = np.zeros(n + 1, dtype=np.int64)                # diagonal d - 2
    E1 = np.full(n + 1, NEG, dtype=np.int64)
    F1 = np.full(n + 1, NEG, dtype=np.int64)
    best = (0, -1, -1)
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - m), min(n, d - 1)           # rows of this diagonal's cells
        i = np.arange(lo, hi + 1)
        j = d - i
        e = np.maximum(E1[i], H1[i] - gap_open) - gap_extend            # (i, j - 1) is on d - 1 in row i
        f = np.maximum(F1[i - 1], H1[i - 1] - gap_open) - gap_extend    # (i - 1, j) is on d - 1 in row i - 1
        h = np.maximum(np.maximum(0, H2[i - 1] + S[ca[i - 1], cb[j - 1]]), np.maximum(e, f))
        H0 = np.zeros(n + 1, dtype=np.int64)            # cells outside the matrix: the boundary's values
        E0 = np.full(n + 1, NEG, dtype=np.int64)
        F0 = np.full(n + 1, NEG, dtype=np.int64)
        H0[i], E0[i], F0[i] = h, e, f
        top = int(h.max())
        if top > 0:
            k = int(np.argmax(h))                       # the first: the smallest i of the diagonal
            cand = (top, int(i[k]) - 1, int(j[k]) - 1)
            if (cand[0], -cand[1], -cand[2]) > (best[0], -best[1], -best[2]):
                best = cand
        H2, H1, E1, F1 = H1, H0, E0, F0
    return best


def align_model(seq: bytes, offsets, pairs, S=S62, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
                max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, sw=sw_numpy) -> np.ndarray:
    """-> ALIGNMENT_DTYPE records in pair order."""
    seq = bytes(seq)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=N.ALIGNMENT_DTYPE)
    memo = {}
    for k, (a, b) in enumerate(pairs):
        pa, pb = seq[offsets[a]:offsets[a + 1]], seq[offsets[b]:offsets[b + 1]]
        if len(pa) * len(pb) > max_cells:
            r = (-1, -1, -1, N.ALIGN_SKIPPED)
        else:
            if (pa, pb) not in memo:
                memo[(pa, pb)] = sw(pa, pb, S, gap_open, gap_extend)
            r = memo[(pa, pb)] + (N.ALIGN_ALIGNED,)
        out[k] = (r[0], self_score(pa, S), self_score(pb, S), r[1], r[2], r[3])
    return out


def kept(score: int, ref: int, min_ratio_pct: int = MIN_RATIO_PCT) -> bool:
    """The edge test of an aligned link."""
    return score >= 1 and 100 * score >= min_ratio_pct * ref


def links(seq: bytes, offsets):
    """The links of cluster_model.cluster_loops, by its own rule: {(m, c): s}, d[p], and the counts that do not depend on the
    edges."""
    seq = bytes(seq)
    n = len(offsets) - 1
    code = {ch: j for j, ch in enumerate(ALPHA)}
    members, d, valid = {}, [0] * n, 0
    for p in range(n):
        s = seq[offsets[p]:offsets[p + 1]]
        own = set()
        for i in range(0, len(s) - M.K):
            w = s[i:i + M.K]
            if any(ch not in code for ch in w):
                continue
            valid += 1
            own.add(w)
        d[p] = len(own)
        for w in own:
            members.setdefault(w, []).append(p)
    length = [int(offsets[p + 1] - offsets[p]) for p in range(n)]
    s_of = {}
    for ps in members.values():
        if len(ps) < 2:
            continue
        c = min(ps, key=lambda p: (-length[p], p))
        for m in ps:
            if m != c:
                s_of[(m, c)] = s_of.get((m, c), 0) + 1
    return s_of, d, dict(valid_windows=valid, pairs=sum(d), kmers=len(members), links=len(s_of))


def cluster_aligned_model(seq: bytes, offsets, min_shared: int = 5, min_cover_pct: int = 20, min_ratio_pct: int = MIN_RATIO_PCT,
                          ref="longer", gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
                          max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS, matrix=None, sw=sw_numpy):
    """-> (FAMILY_DTYPE records, counts, FAMILY_EDGE_DTYPE records, {aligned, cut, skipped, cells}).  sw: the form of the
    recurrence that aligns (a caller that asks for the same pairs many times passes a memoised sw_numpy)."""
    S = S62 if matrix is None else np.asarray(matrix, dtype=np.int64)
    ref = N.ALIGN_REFS.get(ref, ref)
    n = len(offsets) - 1
    s_of, d, counts = links(seq, offsets)
    passing = [(m, c, s) for (m, c), s in sorted(s_of.items()) if s >= min_shared and 100 * s >= min_cover_pct * d[m]]
    aln = align_model(seq, offsets, [(m, c) for m, c, _ in passing], S, gap_open, gap_extend, max_cells, sw)
    edges = np.zeros(len(passing), dtype=N.FAMILY_EDGE_DTYPE)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    best, shared = [-1] * n, [0] * n
    stats = dict(aligned=0, cut=0, skipped=0, cells=0)
    n_kept = 0
    for k, (m, c, s) in enumerate(passing):
        a = aln[k]
        r = int(a["self_a"]) if ref == N.ALIGN_REF_MEMBER else max(int(a["self_a"]), int(a["self_b"]))
        if a["status"] == N.ALIGN_SKIPPED:
            status = N.EDGE_SKIPPED
            stats["skipped"] += 1
        else:
            status = N.EDGE_KEPT if kept(int(a["score"]), r, min_ratio_pct) else N.EDGE_CUT
            stats["aligned"] += 1
            stats["cells"] += int(offsets[m + 1] - offsets[m]) * int(offsets[c + 1] - offsets[c])
            stats["cut"] += status == N.EDGE_CUT
        edges[k] = (m, c, s, a["score"], r, a["end_a"], a["end_b"], status)
        if status == N.EDGE_CUT:
            continue
        n_kept += 1
        if s > shared[m]:                               # ascending c: a tie keeps the smaller c
            best[m], shared[m] = c, s
        x, y = find(m), find(c)
        if x != y:
            parent[max(x, y)] = min(x, y)
    root = [find(p) for p in range(n)]
    counts["edges"] = n_kept
    rec, counts = M._finish(n, root, best, shared, counts)
    return rec, counts, edges, stats


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------

def mutate(rng, p: bytes, rate: float) -> bytes:
    """Substitutions at the given rate, each to a different residue."""
    s = bytearray(p)
    for i in np.flatnonzero(rng.random(len(s)) < rate):
        s[i] = ALPHA[(ALPHA.index(s[i]) + 1 + int(rng.integers(0, 19))) % 20] if s[i] in ALPHA else s[i]
    return bytes(s)


def domain_chain(rng):
    """A centre A + linker + B, a member that is A with every 13th residue substituted and one that is B likewise: each member
    shares its domain's 8-mers with the centre and covers less than half of it.  -> [centre, member A, member B]"""
    a, b = M.random_protein(rng, 120), M.random_protein(rng, 120)

    def sub(p):
        return bytes(ALPHA[(ALPHA.index(ch) + 3) % 20] if i % 13 == 6 else ch for i, ch in enumerate(p))

    return [a + M.random_protein(rng, 30) + b, sub(a), sub(b)]


def two_centres(rng):
    """A member whose link with the most shared 8-mers is to a long two-domain centre (cut by the defaults) and whose other link
    is to a full-length relative (kept).  -> [long centre, relative, member]"""
    a, u, b = M.random_protein(rng, 80), M.random_protein(rng, 60), M.random_protein(rng, 240)
    a_mut = bytes(ALPHA[(ALPHA.index(ch) + 5) % 20] if i % 7 == 3 else ch for i, ch in enumerate(a))       # no 8-mer of a survives
    return [a + M.random_protein(rng, 20) + b, a_mut + u + M.random_protein(rng, 5), a + u]


def alternating_path(rng, n: int):
    """Protein i = segment i + segment i + 1, all 60 long, the shared segment 40 (kept: two thirds of the self-score) or 20
    (cut: one third) in turn, under a random permutation.  -> (list of bytes, the permutation)"""
    segs = [M.random_protein(rng, 40 if i % 2 else 20) for i in range(n + 1)]
    order = rng.permutation(n)
    return [segs[i] + segs[i + 1] for i in order], order
