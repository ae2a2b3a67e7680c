"""Inputs that put kg_proteins_align and the alignment step of kg_proteins_cluster_aligned (kg_align.hpp, kg_host_align.hpp) on
their internal borders, and what they must give where that is known by construction: tests/test_align_edges_host.py checks
tests/align_model.py against these answers on the CPU, tests/test_gpu_align_edges.py checks the device against both.

The borders: a wave owns WAVE = 64 rows of a stripe and reads b and the carry WAVE columns at a time; the stripe carry is in LDS
for b of at most LDS_COLS = 1024 residues and in a slab of device memory beyond; the short launch has at most GRID workgroups
and the long one at most LONG_GRID, fewer when SLAB_BYTES / (8 slab_cols) is smaller, and a workgroup takes pairs from a
counter until none is left; align_cut_kernel counts its three statuses by ballots of WAVE lanes in workgroups of CUT_THREADS.
The numbers below are restated from the two headers; the host test parses the headers and compares."""
from __future__ import annotations

import numpy as np

import align_model as A
import cluster_model as M
from kmergutsjava_amd import _native as N

WAVE = 64                       # kWave: rows of a stripe, columns of a chunk, lanes of a ballot
LDS_COLS = 1024                 # kAlignLdsCols
GRID = 256 * 18                 # kAlignGrid: workgroups of the short launch at most
LONG_GRID = 1024                # kAlignLongGrid
SLAB_BYTES = 256 << 20          # kAlignSlabBytes
CUT_THREADS = 256               # lanes of a workgroup of align_cut_kernel
FILL_A, FILL_B = b"DEK", b"LIV"  # rows, columns: every score between the two sets is negative


# ---- the model, memoised across calls: the pools below are asked for again and again ----------------------------------------

_MEMO = {}


def sw_cached(a: bytes, b: bytes, S=A.S62, gap_open: int = A.GAP_OPEN, gap_extend: int = A.GAP_EXTEND):
    """align_model.sw_numpy, each distinct (a, b, table, gaps) once per process."""
    key = (bytes(a), bytes(b), np.asarray(S, dtype=np.int64).tobytes(), int(gap_open), int(gap_extend))
    if key not in _MEMO:
        _MEMO[key] = A.sw_numpy(a, b, S, gap_open, gap_extend)
    return _MEMO[key]


def model(prots, pairs, matrix=None, gap_open: int = A.GAP_OPEN, gap_extend: int = A.GAP_EXTEND, max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS):
    """align_model.align_model (the numpy form) on a list of proteins.  -> ALIGNMENT_DTYPE records in pair order"""
    seq, off = M.pack(prots)
    return A.align_model(seq, off, pairs, A.S62 if matrix is None else np.asarray(matrix, dtype=np.int64), gap_open, gap_extend, max_cells,
                         sw=sw_cached)


def cluster_model(prots, min_shared: int = 5, min_cover_pct: int = 20, **align):
    """align_model.cluster_aligned_model on a list of proteins.  -> (records, counts, edge records, align counts)"""
    seq, off = M.pack(prots)
    return A.cluster_aligned_model(seq, off, min_shared, min_cover_pct, sw=sw_cached, **align)


def hand_out(prots, pairs, max_cells: int = N.ALIGN_DEFAULT_MAX_CELLS) -> dict:
    """What align_run (kg_host_align.hpp) does with a pair list, restated: which pairs go to which launch, the order they are
    handed out in (descending cells, stable; a skipped pair has 0 cells and is a short one), the two grids and the slab's
    columns.  -> dict(short, long: pair indices in hand-out order; short_grid, long_grid, slab_cols, skipped; n, m: per pair)"""
    length = np.array([len(p) for p in prots], dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n, m = length[pairs[:, 0]], length[pairs[:, 1]]
    skip = n * m > max_cells
    cells = np.where(skip, 0, n * m)
    lng = ~skip & (m > LDS_COLS)

    def order(which):
        idx = np.flatnonzero(which)
        return idx[np.argsort(-cells[idx], kind="stable")]

    short, long = order(~lng), order(lng)
    slab_cols = int((m[lng].max() + WAVE - 1) // WAVE * WAVE) if lng.any() else 0
    long_grid = min(len(long), LONG_GRID, max(1, SLAB_BYTES // (slab_cols * 8))) if len(long) else 0
    return dict(short=short, long=long, short_grid=min(len(short), GRID), long_grid=long_grid, slab_cols=slab_cols,
                skipped=int(skip.sum()), n=n, m=m)


def filler(rng, n: int, letters: bytes) -> bytes:
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=n))


def planted(rng, n: int, letters: bytes, at: dict) -> bytes:
    """n filler residues with the letter at[k] in place k."""
    s = bytearray(filler(rng, n, letters))
    for k, ch in at.items():
        s[k:k + 1] = ch
    assert len(s) == n
    return bytes(s)


# ---- A. a workgroup's second pair ---------------------------------------------------------------------------------------------

SHORT_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 130)
SHORT_A = ((130, 65, 129, 64, 2), (128, 63, 127, 1, 65))        # the first proteins: five relatives of one base, five random
SHORT_B = ((129, 64, 130, 63, 1), (127, 65, 128, 2, 130))       # the second proteins likewise
SHORT_PAIRS = GRID + 400
SHORT_MAX_CELLS = 129 * 130     # 130 x 130 alone is more: of the pairs drawn below, one in 24 is skipped


def short_pool():
    """10 + 10 proteins; 0 .. 9 are first proteins (a), 10 .. 19 second ones (b); 0 .. 4 and 10 .. 14 are mutated heads of one base."""
    rng = np.random.default_rng(11)
    base = M.random_protein(rng, 130)
    return ([A.mutate(rng, base[:k], 0.15) for k in SHORT_A[0]] + [M.random_protein(rng, k) for k in SHORT_A[1]] +
            [A.mutate(rng, base[:k], 0.15) for k in SHORT_B[0]] + [M.random_protein(rng, k) for k in SHORT_B[1]])


def _short_pairs(rng, count: int):
    """count pairs of the short pool: the 100 distinct ones, then pairs at random of an a of more than one stripe and a b of 63
    residues or more, so that the pairs with the fewest cells behind the 100 still have a second stripe."""
    full = np.array([(i, 10 + j) for i in range(10) for j in range(10)])
    rows = np.array([i for i, k in enumerate(SHORT_A[0] + SHORT_A[1]) if k > WAVE])
    cols = np.array([10 + j for j, k in enumerate(SHORT_B[0] + SHORT_B[1]) if k >= WAVE - 1])
    rest = np.stack([rng.choice(rows, size=count - len(full)), rng.choice(cols, size=count - len(full))], axis=1)
    return np.concatenate([full, rest])


def second_pair_short():
    """GRID + 400 pairs of the short pool in a random order: more pairs than the short launch has workgroups, so the 400 pairs
    with the fewest cells are taken by a workgroup that has done one.  Those are the skipped pairs (0 cells: handed out last,
    about 200: a tenth of all would be more than 400 and leave no second pair that aligns), the pairs of one or two residues
    and some 100 pairs of 65 x 63.  -> (proteins, pairs, max_cells)"""
    rng = np.random.default_rng(12)
    pairs = _short_pairs(rng, SHORT_PAIRS)
    return short_pool(), pairs[rng.permutation(len(pairs))], SHORT_MAX_CELLS


LONG_A, LONG_B = (129, 65, 64, 1), (1025, 1087, 1088, 1089)
LONG_PAIRS = LONG_GRID + 76
# pairs per length of a: the LONG_GRID pairs with the most cells all have 129 rows (three stripes: rows 63 and 127 go through the
# slab), so a pair of 65 rows that is handed out behind them goes to a workgroup whose slab holds a 129-row pair's row 127
LONG_COUNT = {129: LONG_GRID, 65: 76 - 8, 64: 4, 1: 4}
LONG_SHORT_PAIRS = 300


def second_pair_long():
    """LONG_GRID + 76 long pairs (b: mutated heads of one base of 1089 residues, a: mutated pieces of it from residue 896 on: 129 rows end in column 1024) with 300
    short pairs shuffled in between: proteins 0 .. 19 are the short pool, 20 .. 23 the a, 24 .. 27 the b.
    -> (proteins, pairs)"""
    rng = np.random.default_rng(13)
    base = M.random_protein(rng, max(LONG_B))
    a = [A.mutate(rng, base[896:896 + k], 0.15) for k in LONG_A]
    b = [A.mutate(rng, base[:k], 0.15) for k in LONG_B]
    long_pairs = [(20 + i, 24 + k % 4) for i, rows in enumerate(LONG_A) for k in range(LONG_COUNT[rows])]
    pairs = np.concatenate([np.array(long_pairs), _short_pairs(rng, LONG_SHORT_PAIRS)])
    assert len(long_pairs) == LONG_PAIRS
    return short_pool() + a + b, pairs[rng.permutation(len(pairs))]


# ---- B. the LDS / slab border -------------------------------------------------------------------------------------------------

BORDER_M = (LDS_COLS - 1, LDS_COLS, LDS_COLS + 1)
BORDER_N = (1, 64, 65, 129, 193)
BORDER_INSERT = 12


def border_pairs():
    """For each b of 1023, 1024, 1025 random residues, five a: b's last residue (1 row), and for 64, 65, 129, 193 rows b's last
    n - 12 residues with 12 W put in, at rows 58 .. 69 in the a of 129 and 193 rows (a vertical gap across the first stripe
    border: its F goes through the carry) and at rows 26 .. 37 in the a of 64 and 65 rows, which have no residues behind row 69.  The answer, asserted on the model: the whole of a
    with one gap, score = self(the copied residues) - (11 + 12), ending in a's last row and b's LAST column.
    -> (proteins, pairs, [(score, end_a, end_b)] for the pairs with a gap, None for the one-row pairs)"""
    rng = np.random.default_rng(21)
    prots, pairs, want = [], [], []
    for m in BORDER_M:
        b = M.random_protein(rng, m).replace(b"W", b"A").replace(b"Y", b"A").replace(b"F", b"A")     # nothing W scores against
        prots.append(b)
        at_b = len(prots) - 1
        for n in BORDER_N:
            if n == 1:
                prots.append(b[-1:])
                want.append(None)
            else:
                piece, at = b[m - (n - BORDER_INSERT):], 58 if n >= 2 * WAVE else 26
                prots.append(piece[:at] + b"W" * BORDER_INSERT + piece[at:])
                want.append((A.self_score(piece) - (A.GAP_OPEN + BORDER_INSERT * A.GAP_EXTEND), n - 1, m - 1))
            assert len(prots[-1]) == n
            pairs.append((len(prots) - 1, at_b))
    return prots, pairs, want


LAST_COLUMN = [(row, m) for row in (WAVE - 1, WAVE, 129) for m in (LDS_COLS, LDS_COLS + 1)]


def last_column_case(row: int, m: int):
    """Six W that end in row `row` of a (130 rows) and in b's last column, fillers elsewhere.  -> (a, b, (66, row, m - 1))"""
    rng = np.random.default_rng(22)
    a = filler(rng, row - 5, FILL_A) + b"WWWWWW" + filler(rng, 130 - row - 1, FILL_A)
    b = filler(rng, m - 6, FILL_B) + b"WWWWWW"
    assert len(a) == 130 and len(b) == m
    return a, b, (66, row, m - 1)


GAP_COLUMNS = (LDS_COLS - 1, LDS_COLS)


def vertical_gap_case(col: int):
    """a = p with 11 W put in behind its residue 59 (rows 60 .. 70: across the stripe border), b = col - 59 unrelated
    residues and then p: the gap's cells are all in column `col`, whose carry is the last one that would fit LDS (1023) or the
    first that does not (1024).  -> (a, b, (self(p) - 22, 210, col + 140))"""
    rng = np.random.default_rng(23)
    p = M.random_protein(rng, 200)
    a = p[:60] + b"W" * 11 + p[60:]
    b = filler(rng, col - 59, FILL_B) + p
    assert b.index(p[:60]) + 59 == col
    return a, b, (A.self_score(p) - 22, 210, col + 140)


def horizontal_gap_case():
    """a = p, b = 938 unrelated residues, p's first 80, 12 W, p's rest: the gap lies in row 79 (the second stripe) over the
    columns 1018 .. 1029, on both sides of column 1023 / 1024.  -> (a, b, (self(p) - 23, 199, 1149))"""
    rng = np.random.default_rng(24)
    p = M.random_protein(rng, 200)
    b = filler(rng, LDS_COLS - 6 - 80, FILL_B) + p[:80] + b"W" * 12 + p[80:]
    assert b.index(b"W" * 12) == LDS_COLS - 6
    return p, b, (A.self_score(p) - 23, 199, len(b) - 1)


# ---- C. the slab-bytes cap and the stride -------------------------------------------------------------------------------------

CAP_COLS = 40000                # one b of this many residues: slab_cols = 40000, and 256 MiB / (8 * 40000) = 838 workgroups
CAP_LONG_PAIRS = 900
CAP_A, CAP_B = (65, 129, 65, 129), (1025, 1100, 1025, 1100)


def slab_cap_case():
    """One pair of 1 x 40000 and 900 long pairs of a pool of 4 x 4 (a of 65 and 129 rows, mutated pieces of the base of the b
    of 1025 and 1100): the long launch has SLAB_BYTES / (8 * 40000) workgroups, fewer than pairs, and each of them carries
    at slab + blockIdx.x * 40000.  Protein 0 is the one residue, 1 the long b, 2 .. 5 the a, 6 .. 9 the b.  -> (proteins, pairs)"""
    rng = np.random.default_rng(31)
    base = M.random_protein(rng, max(CAP_B))
    a = [A.mutate(rng, base[940:940 + k], 0.15) for k in CAP_A]
    b = [A.mutate(rng, base[:k], 0.15) for k in CAP_B]
    pairs = np.array([(2 + k % 4, 6 + (k // 4) % 4) for k in range(CAP_LONG_PAIRS)] + [(0, 1)])
    return [b"W", M.random_protein(rng, CAP_COLS)] + a + b, pairs[rng.permutation(len(pairs))]


# ---- D. ties of the best cell ---------------------------------------------------------------------------------------------------

TIE_ROWS = ((5, 69), (10, 67), (63, 64), (0, 129), (64, 127))
TIE_COLS = ((89, 0), (64, 63), (65, 1), (0, 89))
TIE_COLS_LONG = ((LDS_COLS, 0), (1, LDS_COLS - 1), (64, 63))
TIE_N, TIE_M = 130, 90


def _tie(name, rows: dict, cols: dict, m: int, want):
    rng = np.random.default_rng(len(name) + 1000 * m + sum(rows) + 7 * sum(cols))
    return name, planted(rng, TIE_N, FILL_A, rows), planted(rng, m, FILL_B, cols), want


def tie_cases():
    """P and Y planted among fillers: S[P, P] = S[Y, Y] = 7 and everything else about them is negative, so the cells of score 7
    are exactly the (row, column) pairs that hold the same letter, none lies diagonally behind another, and the answer is the
    one with the smallest row, then the smallest column.  -> [(name, a, b, (7, i, j))]"""
    out = []
    for m, grid in ((TIE_M, TIE_COLS), (LDS_COLS + 1, TIE_COLS_LONG)):
        for i1, i2 in TIE_ROWS:
            for j1, j2 in grid:
                out.append(_tie("rows %d %d cols %d %d of %d" % (i1, i2, j1, j2, m), {i1: b"P", i2: b"Y"}, {j1: b"P", j2: b"Y"}, m, (7, i1, j1)))
        last = m - 1
        # one row, two columns: in two chunks of 64 columns (row 69 is lane 5: steps 8 and 75), in one chunk, and with the last column
        out.append(_tie("row 69 cols 70 3 of %d" % m, {69: b"P"}, {70: b"P", 3: b"P"}, m, (7, 69, 3)))
        out.append(_tie("row 69 cols 20 40 of %d" % m, {69: b"P"}, {20: b"P", 40: b"P"}, m, (7, 69, 20)))
        out.append(_tie("row 69 cols last 66 of %d" % m, {69: b"P"}, {last: b"P", 66: b"P"}, m, (7, 69, 66)))
        # three cells: the smallest row has the largest column; the two others share a column in two stripes
        out.append(_tie("three: rows 3 67 129 of %d" % m, {3: b"Y", 67: b"P", 129: b"P"}, {2: b"P", last: b"Y"}, m, (7, 3, last)))
        out.append(_tie("three: rows 64 65 128 of %d" % m, {64: b"P", 65: b"Y", 128: b"P"}, {last - 1: b"P", 0: b"Y"}, m, (7, 64, last - 1)))
        # four cells: one lane's two rows against two columns
        out.append(_tie("four: rows 5 69 cols 70 3 of %d" % m, {5: b"P", 69: b"P"}, {70: b"P", 3: b"P"}, m, (7, 5, 3)))
    return out


# ---- E. bytes and tables --------------------------------------------------------------------------------------------------------

def byte_proteins():
    """All 256 byte values ascending, the same descending, and 300 random residues.  -> (proteins, pairs: every ordered pair)"""
    every = bytes(range(256))
    return [every, every[::-1], M.random_protein(np.random.default_rng(51), 300)], [(a, b) for a in range(3) for b in range(3)]


def tables():
    """name -> (21 x 21 table, gap_open, gap_extend): the bounds -16 and 16 of an entry, and a positive "everything else" row."""
    rng = np.random.default_rng(52)
    flat = np.full((21, 21), 16, dtype=np.int64)
    diag = np.full((21, 21), -16, dtype=np.int64)
    np.fill_diagonal(diag, 16)
    upper = np.triu(rng.integers(-16, 17, size=(21, 21)))
    rand = upper + np.triu(upper, 1).T
    rand[20, :] = rand[:, 20] = rng.integers(1, 17, size=21)
    return {"16 everywhere": (flat, A.GAP_OPEN, A.GAP_EXTEND), "16 and -16": (diag, A.GAP_OPEN, A.GAP_EXTEND),
            "16 and -16, gaps 0 and 1": (diag, 0, 1), "random, everything else positive": (rand, A.GAP_OPEN, A.GAP_EXTEND)}


# ---- F. the cut kernel ------------------------------------------------------------------------------------------------------------

CUT_L = (1, 63, 64, 65, 255, 256, 257, 513)
CUT_MAX_CELLS = 12000
CUT_KINDS = ("kept", "cut", "member", "skipped")
# a link's status by its kind, under ref = longer and ref = member, at min_ratio_pct = 50
CUT_STATUS = {"longer": dict(kept=N.EDGE_KEPT, cut=N.EDGE_CUT, member=N.EDGE_CUT, skipped=N.EDGE_SKIPPED),
              "member": dict(kept=N.EDGE_KEPT, cut=N.EDGE_CUT, member=N.EDGE_KEPT, skipped=N.EDGE_SKIPPED)}
_CUT_TAIL = dict(kept=10, cut=70, member=80, skipped=300)        # what a centre holds behind the 40 shared residues


def cut_links(L: int):
    """Exactly L links that pass the 8-mer tests (5, 20), each from a member of its own to one of at most 8 centres, in the
    spirit of align_model.alternating_path.  A centre is 40 residues S and a random tail, and it is the longest protein that
    holds S's 8-mers; a member holds a piece of one S and no other valid 8-mer.  By the kind of the pair:
      kept     S + 10: the member is S[:40], S[:39] or S[1:40] and scores its self-score, four fifths of the centre's
      cut      S + 70: the member is 20 or 21 residues of S and 80 more with an X in every fourth place (no 8-mer, but 60
               residues of self-score), so it scores a quarter of its own self-score and less of the centre's
      member   S + 80: the member is a piece of S as for kept; a third of the centre's self-score, all of its own
      skipped  S + 300: 39 or 40 rows against 340 columns are more than CUT_MAX_CELLS = 12000 cells; every other pair has fewer
    Member k's kind is CUT_KINDS[k % 4]; the proteins are then numbered by a random permutation, so that in the order of the
    links (ascending member) the statuses follow no period.  The pool of contents is the same for every L: 2 x 4 centres and 3
    members of each.  -> (proteins, the kind of every link in link order)"""
    rng = np.random.default_rng(41)
    shared = [[M.random_protein(rng, 40) for _ in CUT_KINDS] for _ in range(2)]
    centre = [[shared[g][k] + M.random_protein(rng, _CUT_TAIL[kind]) for k, kind in enumerate(CUT_KINDS)] for g in range(2)]
    junk = []
    for _ in range(6):
        j = bytearray(M.random_protein(rng, 80))
        j[0::4] = b"X" * 20
        junk.append(bytes(j))
    prots, kinds, used = [], [], {}
    for i in range(L):
        k, v, g = i % 4, (i // 4) % 3, (i // 12) % 2
        s = shared[g][k]
        if CUT_KINDS[k] == "cut":
            prots.append((s[:20], s[:21], s[1:21])[v] + junk[3 * g + v])
        else:
            prots.append((s[:40], s[:39], s[1:40])[v])
        kinds.append(CUT_KINDS[k])
        used[(g, k)] = centre[g][k]
    kinds += [None] * len(used)
    prots += list(used.values())
    where = np.random.default_rng(4100 + L).permutation(len(prots))         # protein `where[x]` is item x
    out, kind_of = [None] * len(prots), [None] * len(prots)
    for x, at in enumerate(where):
        out[at], kind_of[at] = prots[x], kinds[x]
    return out, [k for k in kind_of if k is not None]


HALF_MATRIX = np.full((21, 21), -3, dtype=np.int64)
np.fill_diagonal(HALF_MATRIX, 2)
HALF_GAPS = dict(gap_open=5, gap_extend=2)


def half_cases():
    """Under +2 / -3 (gaps 5 and 2) a member and a centre that share their first 20 residues and nothing else score 40.
    -> {name: ([member, centre], ref, (score, self of the member, self of the centre))}
      longer: the centre's self-score, 80, is the larger: 100 * 40 == 50 * 80
      member: the member's self-score is 80 and the centre's 100: 100 * 40 == 50 * 80 under ref = member, and under
              ref = longer the bound lies at 40"""
    rng = np.random.default_rng(42)
    head = M.random_protein(rng, 20).replace(b"M", b"A").replace(b"W", b"C")
    return {"longer": ([head + b"M" * 19, head + b"W" * 20], "longer", (40, 78, 80)),
            "member": ([head + b"M" * 20, head + b"W" * 30], "member", (40, 80, 100))}


MINUS_ONE = np.full((21, 21), -1, dtype=np.int64)


def identical_pair():
    """Two identical proteins: one link, every 8-mer shared; under MINUS_ONE they score 0."""
    p = M.random_protein(np.random.default_rng(43), 40)
    return [p, p]


BEST_PARAMS = dict(min_cover_pct=10, min_ratio_pct=15)


def best_after_cut_case(member_first: bool):
    """A member = B1 (25) + B2 (25) + A (40) + 5 residues of its own, and three longer centres: one holds A and 360 other residues
    (33 shared 8-mers, a tenth of its self-score: cut at 15 %), two hold B1 or B2 and 80 or 81 others (18 shared 8-mers each, a
    quarter: kept).  best is the smaller of the two kept centres, shared 18.
    -> (proteins, the member's index, [the centres: kept, cut, kept])"""
    rng = np.random.default_rng(44)
    b1, b2, a = M.random_protein(rng, 25), M.random_protein(rng, 25), M.random_protein(rng, 40)
    member = b1 + b2 + a + M.random_protein(rng, 5)
    centres = [b2 + M.random_protein(rng, 81), a + M.random_protein(rng, 360), b1 + M.random_protein(rng, 80)]
    return ([member] + centres, 0, [1, 2, 3]) if member_first else (centres + [member], 3, [0, 1, 2])
