"""kg_proteins_align_paths and kg_proteins_search_paths on the GPU against tests/trace_model.py, byte for byte
(include/kmerguts_hip.h states the rule).  The shapes follow the constants of kg_trace.hpp and kg_host_trace.hpp: the 64-row
stripe, eight steps to a direction word, the slab sizes that split the two launches, and the grids."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_model as A
import cluster_model as M
import search_model as S
import trace_model as T
from kmergutsjava_amd import _native as N
from kmergutsjava_amd import align_scores as AS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
_DEV, _HOST = open(os.path.join(_CSRC, "kg_trace.hpp")).read(), open(os.path.join(_CSRC, "kg_host_trace.hpp")).read()


def _const(text, name):
    """A constant of the headers: `N`, `A * B` or `A << B`, with or without a u / ull suffix; anything else is an error."""
    expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)
    m = re.fullmatch(r"(\d+)(?:ull|u)?(?: (\*|<<) (\d+)(?:ull|u)?)?", expr.strip())
    assert m, (name, expr)
    a, op, b = int(m.group(1)), m.group(2), m.group(3)
    return a if op is None else a * int(b) if op == "*" else a << int(b)


WAVE = _const(open(os.path.join(_CSRC, "kg_device.hpp")).read(), "kWave")
WORD = _const(_DEV, "kTraceCellsPerWord")                  # steps of one direction word
GRID, LONG_GRID = _const(_HOST, "kTraceGrid"), _const(_HOST, "kTraceLongGrid")
SHORT_SLAB, SLAB = _const(_HOST, "kTraceShortSlabBytes"), _const(_HOST, "kTraceSlabBytes")
LDS_COLS = N.ALIGN_LDS_COLS
FILL_A, FILL_B = b"KR", b"LIV"              # every score between the two sets is negative, in BLOSUM62 and in +2 / -3
M23 = np.full((21, 21), -3, dtype=np.int64)
np.fill_diagonal(M23, 2)
M23[20, 20] = -3


def test_the_constants():
    assert (WAVE, WORD) == (64, 8) and GRID >= 1024 and LONG_GRID >= 1 and SHORT_SLAB < SLAB
    assert all(A.S62[AS.ALPHA.index(x), AS.ALPHA.index(y)] < 0 for x in FILL_A for y in FILL_B + b"ACD")


def _filler(rng, n, letters):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=n))


def _paths(prots, pairs, **kw):
    from kmergutsjava_amd import hotpath
    seq, off = M.pack(prots)
    return hotpath.align_proteins(seq, off, pairs, paths=True, **kw)


def _invariant(aln, pth):
    """The residue columns counted along a equal those counted along b, on every traced record."""
    t = pth["status"] == N.PATH_TRACED
    ra = (aln["end_a"] - pth["start_a"] + 1) - pth["gap_cols_b"]
    rb = (aln["end_b"] - pth["start_b"] + 1) - pth["gap_cols_a"]
    assert (ra[t] == rb[t]).all() and (ra[t] >= 1).all() and (pth["identical"][t] <= ra[t]).all() and (pth["positive"][t] <= ra[t]).all()
    assert (pth["start_a"][~t] == -1).all() and (pth["start_b"][~t] == -1).all()


def _same(prots, pairs, matrix=None, gap_open=11, gap_extend=1, max_cells=N.ALIGN_DEFAULT_MAX_CELLS, max_trace_cells=N.TRACE_DEFAULT_MAX_CELLS):
    """The device's alignment and path records == the models'.  -> (alignment records, path records)"""
    seq, off = M.pack(prots)
    Smat = A.S62 if matrix is None else np.asarray(matrix)
    want = A.align_model(seq, off, pairs, Smat, gap_open, gap_extend, max_cells)
    wpth = T.paths_model(seq, off, pairs, want, Smat, gap_open, gap_extend, max_trace_cells)
    got, pth = _paths(prots, pairs, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, max_cells=max_cells, max_trace_cells=max_trace_cells)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:5]
    bad = np.flatnonzero(pth != wpth)
    assert pth.tobytes() == wpth.tobytes(), (bad[:5], pth[bad[:5]], wpth[bad[:5]], got[bad[:5]])
    _invariant(got, pth)
    return got, pth


# ---- shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("related", [True, False])
def test_every_box_of_130_by_140(related):
    """a of 1 to 130 residues crossed with b of 1 to 140: the prefixes of one protein against the prefixes of another, so that one
    pair of tables holds every pair's (a box of the whole matrix has the whole matrix's values), and a path depends only on its
    end cell.  The boxes' columns cover a stripe's step count of 8k - 1, 8k and 8k + 1 many times."""
    rng = np.random.default_rng(41)
    a = M.random_protein(rng, 130)
    b = (A.mutate(rng, a[:50], 0.1) + M.random_protein(rng, 7) + A.mutate(rng, a[50:90], 0.1) + A.mutate(rng, a[95:], 0.1) + M.random_protein(rng, 8))[:140] \
        if related else M.random_protein(rng, 140)
    assert len(b) == 140
    prots = [a[:n] for n in range(1, 131)] + [b[:m] for m in range(1, 141)]
    pairs = np.array([(n - 1, 130 + m - 1) for n in range(1, 131) for m in range(1, 141)])
    ca, cb = T._codes(a), T._codes(b)
    H, E, F = T.tables_numpy(ca, cb, A.S62, 11, 1)
    Hn = np.asarray(H)
    H, E, F = Hn.tolist(), np.asarray(E).tolist(), np.asarray(F).tolist()
    want = np.zeros(len(pairs), dtype=N.ALIGN_PATH_DTYPE)
    ends = np.zeros((len(pairs), 3), dtype=np.int64)
    memo = {}
    for k, (n, m) in enumerate((n, m) for n in range(1, 131) for m in range(1, 141)):
        box = Hn[1:n + 1, 1:m + 1]
        at = int(np.argmax(box))                        # row-major: the smallest i, then the smallest j
        i, j = divmod(at, m)
        score = int(box[i, j])
        ends[k] = (score, i, j) if score > 0 else (0, -1, -1)
        if score <= 0:
            want[k] = T.NO_PATH + (N.PATH_NONE,)
            continue
        if (i, j) not in memo:
            memo[(i, j)] = T.walk(H, E, F, ca, cb, A.S62, 11, 1, i, j)[0]
        want[k] = memo[(i, j)] + (N.PATH_TRACED,)
    got, pth = _paths(prots, pairs)
    assert (got["score"] == ends[:, 0]).all() and (got["end_a"] == ends[:, 1]).all() and (got["end_b"] == ends[:, 2]).all()
    bad = np.flatnonzero(pth != want)
    assert pth.tobytes() == want.tobytes(), (bad[:5], pairs[bad[:5]], pth[bad[:5]], want[bad[:5]])
    _invariant(got, pth)
    steps = got["end_b"][pth["status"] == 0] + 1 + WAVE - 1
    assert all((steps % WORD == r).sum() >= (500 if related else 1) for r in (WORD - 1, 0, 1)), np.bincount(steps % WORD)
    if related:
        assert (pth["gap_opens"] > 0).sum() > 1000 and len(memo) > 100, ((pth["gap_opens"] > 0).sum(), len(memo))
        # the slice the model's own fill gives for a few boxes: the prefix argument above is not the only witness
        few = np.array([0, 77, 9000, 18199, 12345])
        seq, off = M.pack(prots)
        assert T.paths_model(seq, off, pairs[few], got[few]).tobytes() == want[few].tobytes()


@pytest.mark.parametrize("row,length", [(0, 64), (0, 65), (63, 1), (63, 2), (64, 66), (65, 30), (64, 1)])
def test_start_and_end_rows_by_construction(row, length):
    """A segment planted at row `row` of a and column 0 of b: the path starts at (row, 0) and ends `length` cells down the diagonal,
    in the last row of a or before it."""
    rng = np.random.default_rng(42)
    q = M.random_protein(rng, length).replace(b"R", b"A").replace(b"K", b"C").replace(b"L", b"A").replace(b"I", b"C").replace(b"V", b"D")
    for tail in (0, 70):
        a = _filler(rng, row, FILL_A) + q + _filler(rng, tail, FILL_A)
        b = q + _filler(rng, 20, FILL_B)
        got, pth = _same([a, b], [(0, 1), (1, 0)])
        assert (got["end_a"][0], got["end_b"][0]) == (row + length - 1, length - 1)
        assert pth[0].tolist() == (row, 0, length, length, 0, 0, 0, 0) and pth[1].tolist() == (0, row, length, length, 0, 0, 0, 0)


def test_gaps_across_stripe_borders():
    rng = np.random.default_rng(43)
    p = M.random_protein(rng, 200)
    ins = lambda k: _filler(rng, k, b"W")                       # W against anything but W, Y, F is negative: the insert is a gap
    v11 = p[:60] + ins(11) + p[60:]                             # a vertical gap (F) over rows 60 .. 70
    v130 = p[:40] + ins(130) + p[40:]                           # ... and one of 130 rows: two borders
    h100 = p[:80] + ins(100) + p[80:]                           # a horizontal gap (E) of 100 columns
    got, pth = _same([p, v11, v130, h100], [(1, 0), (2, 0), (0, 3), (3, 0), (0, 1), (0, 2), (0, 0)])
    assert pth["gap_opens"].tolist() == [1, 1, 1, 1, 1, 1, 0]
    assert pth["gap_cols_b"].tolist() == [11, 130, 0, 100, 0, 0, 0] and pth["gap_cols_a"].tolist() == [0, 0, 100, 0, 11, 130, 0]
    assert (pth["start_a"] == 0).all() and (pth["start_b"] == 0).all() and (pth["identical"] == 200).all()


def test_horizontal_gaps_at_every_place_in_a_word_and_across_a_chunk():
    """b = s filler columns + p[:c] + g W's + p[c:]: the gap runs in row c - 1 over columns s + c .. s + c + g - 1, at steps
    t = column + (c - 1) % 64."""
    rng = np.random.default_rng(44)
    p = M.random_protein(rng, 110).replace(b"W", b"A")
    cases = [(c, s, g) for c in (33, 34, 35, 36) for s in (0, 1) for g in (9, 16)] + [(60, 0, 10), (60, 1, 10), (20, 0, 50)]
    prots, pairs, first, last = [p], [], set(), set()
    for c, s, g in cases:
        prots.append(_filler(rng, s, FILL_B) + p[:c] + b"W" * g + p[c:])
        pairs.append((0, len(prots) - 1))
        t0 = s + c + (c - 1) % WAVE
        first.add(t0 % WORD)
        last.add((t0 + g - 1) % WORD)
    assert {0, WORD - 1} <= first and {0, WORD - 1} <= last
    got, pth = _same(prots, pairs)
    assert pth["gap_cols_a"].tolist() == [g for _, _, g in cases] and (pth["gap_opens"] == 1).all() and (pth["gap_cols_b"] == 0).all()
    assert pth["start_b"].tolist() == [s for _, s, _ in cases]


@pytest.mark.parametrize("m", [LDS_COLS - 1, LDS_COLS, LDS_COLS + 1])
def test_long_columns_with_the_path_in_the_last_column(m):
    """b of 1023, 1024 and 1025 residues (the last one carries its stripes in device memory and runs in the second launch)
    against a of 1, 64, 65 and 129 whose last residues are b's last."""
    rng = np.random.default_rng(45)
    b = M.random_protein(rng, m - 1).replace(b"W", b"A") + b"W"
    prots, pairs = [b], []
    for n in (1, 64, 65, 129):
        tail = b[-min(n, 30):]
        prots.append(_filler(rng, n - len(tail), FILL_A) + tail)
        pairs.append((len(prots) - 1, 0))
    got, pth = _same(prots, pairs)
    assert (got["end_b"] == m - 1).all() and got["end_a"].tolist() == [0, 63, 64, 128] and (pth["status"] == 0).all()
    assert pth["identical"][0] == 1 and (pth["identical"][1:] >= 30).all() and (pth["start_a"][1:] <= np.array([34, 35, 99])).all()


# ---- ties -------------------------------------------------------------------------------------------------------------------

TIE_CASES = [   # (a, b, gap_open, gap_extend, the 0-based row of the tie cell, the record, the tie): tests/test_trace_host.py works them out
    (b"ACAA", b"ACCAA", 0, 2, 1, (1, 2, 3, 3, 0, 0, 0), "diagonal = E"),
    (b"ACCAA", b"ACAA", 0, 2, 2, (2, 1, 3, 3, 0, 0, 0), "diagonal = F"),
    (b"ACD", b"CAD", 0, 1, 1, (1, 0, 2, 2, 1, 1, 0), "E = F"),
    (b"CACDAACC", b"CADCCAAC", 1, 1, 3, (0, 0, 6, 6, 1, 1, 0), "all three"),
    (b"AAAA", b"AACCAA", 0, 1, 1, (0, 0, 4, 4, 1, 2, 0), "E open = extend"),
    (b"AACCAA", b"AAAA", 0, 1, 3, (0, 0, 4, 4, 1, 0, 2), "F open = extend"),
]


@pytest.mark.parametrize("lane", [0, WAVE - 1])
def test_the_preferences_at_lane_0_and_at_lane_63(lane):
    """Each hand-worked tie behind filler rows, so that the tie's cell is in the first or the last lane of the second stripe,
    and behind 0 and 5 filler columns."""
    rng = np.random.default_rng(46)
    for a, b, go, ge, tie_row, rec, kind in TIE_CASES:
        for cols in (0, 5):
            rows = WAVE + lane - tie_row
            pa, pb = _filler(rng, rows, FILL_A) + a, _filler(rng, cols, FILL_B) + b
            ties = {}
            end, wrec = T.trace_numpy(pa, pb, M23, go, ge, ties=ties)
            assert wrec == (rec[0] + rows, rec[1] + cols) + rec[2:] and kind in ties, (a, b, wrec, ties)
            got, pth = _same([pa, pb], [(0, 1)], matrix=M23, gap_open=go, gap_extend=ge)
            assert pth[0].tolist() == wrec + (0,)


@pytest.mark.parametrize("matrix,gap_open,gap_extend", [(M23, 5, 2), (M23, 0, 1), (None, 0, 1), (M23, 0, 2), (None, 2 ** 31 - 1, 2 ** 31 - 1),
                                                         (M23, 2 ** 31 - 1, 1)])
def test_relatives_of_few_letters_under_other_costs(matrix, gap_open, gap_extend):
    """Three-letter proteins of up to 150 residues with deletions: equal scores everywhere, across two stripe borders."""
    rng = np.random.default_rng(47)
    prots = []
    for _ in range(6):
        base = _filler(rng, int(rng.integers(100, 151)), b"ACD")
        cut = int(rng.integers(10, 80))
        prots += [base, base[:cut] + base[cut + int(rng.integers(1, 6)):], A.mutate(rng, base, 0.1)[int(rng.integers(0, 9)):]]
    pairs = [(3 * k + x, 3 * k + y) for k in range(6) for x, y in ((0, 1), (1, 0), (0, 2), (2, 1))]
    got, pth = _same(prots, pairs, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend)
    assert (pth["status"] == 0).all() and ((pth["gap_opens"] > 0).sum() > 6) == (gap_open < 2 ** 31 - 1)


# ---- slab reuse and hand-out ------------------------------------------------------------------------------------------------

N_LARGE, N_SMALL, N_NONE = GRID, 400, 300


@pytest.fixture(scope="module")
def short_pairs():
    """Grid pairs of relatives of 42 to 48 residues, 400 pairs of pieces of at most 20 residues of the same relatives, and 300
    pairs without a path (X's and an empty protein), shuffled.  Every pair of the first two kinds is traced (its_box > 0), and
    every box of the second kind is smaller than every box of the first: handed out in descending order of the boxes, positions
    Grid .. Grid + 399 are traced in slabs that a larger box has used."""
    rng = np.random.default_rng(48)
    base = M.random_protein(rng, 48)
    large = [A.mutate(rng, base, 0.1)[int(rng.integers(0, 6)):] for _ in range(10)]
    small = [p[int(rng.integers(0, 6)):][:int(rng.integers(12, 21))] for p in large]
    prots = large + small + [b"XXXX", b""]
    pairs = np.concatenate([rng.integers(0, 10, size=(N_LARGE, 2)), rng.integers(10, 20, size=(N_SMALL, 2)),
                            np.stack([rng.integers(0, 22, size=N_NONE), rng.integers(20, 22, size=N_NONE)], axis=1)])
    pairs = pairs[rng.permutation(len(pairs))]
    seq, off = M.pack(prots)
    aln = A.align_model(seq, off, pairs)
    return prots, pairs, aln, T.paths_model(seq, off, pairs, aln)


def test_the_hand_out_order_of_the_short_pairs(short_pairs):
    """From the model's box cells, in the order trace_run hands the pairs out (descending box cells, stable): the first Grid
    positions are traced pairs, the next 400 are traced pairs too and each has a smaller box than every one of the first Grid,
    the pairs without a path come last."""
    prots, pairs, aln, want = short_pairs
    box = np.where(aln["score"] > 0, (aln["end_a"].astype(np.int64) + 1) * (aln["end_b"].astype(np.int64) + 1), 0)
    order = np.argsort(-box, kind="stable")
    first, second, rest = order[:GRID], order[GRID:GRID + N_SMALL], order[GRID + N_SMALL:]
    assert (want["status"][first] == N.PATH_TRACED).all() and (want["status"][second] == N.PATH_TRACED).all()
    assert 0 < box[second].min() and box[second].max() < box[first].min(), (box[second].max(), box[first].min())
    assert (want["status"][rest] == N.PATH_NONE).all() and (box[rest] == 0).all() and len(rest) == N_NONE
    words = lambda k: -(-(int(aln["end_a"][k]) + 1) // WAVE) * (-(-(int(aln["end_b"][k]) + WAVE) // WORD)) * WAVE * 4
    assert max(words(k) for k in order[:GRID + N_SMALL]) <= SHORT_SLAB      # all of them in the wide launch, Grid workgroups


def test_more_pairs_than_workgroups_twice_and_reversed(short_pairs):
    """Grid + 400 traced pairs in descending order of their boxes (test_the_hand_out_order_of_the_short_pairs): a workgroup that
    takes a second pair traces it in the slab of a larger one, uncleared."""
    prots, pairs, aln, want = short_pairs
    for _ in range(2):
        got, pth = _paths(prots, pairs)
        assert got.tobytes() == aln.tobytes() and pth.tobytes() == want.tobytes(), np.flatnonzero(pth != want)[:5]
    got, pth = _paths(prots, pairs[::-1])
    assert got.tobytes() == aln[::-1].tobytes() and pth.tobytes() == want[::-1].tobytes()
    assert (want["status"] == N.PATH_TRACED).sum() == GRID + N_SMALL and (want["status"] == N.PATH_NONE).sum() == N_NONE
    _invariant(aln, want)


def test_a_pair_over_max_trace_cells_beside_traced_ones(short_pairs):
    prots, pairs, aln, _ = short_pairs
    sub = pairs[:300]
    box = (aln["end_a"][:300].astype(np.int64) + 1) * (aln["end_b"][:300] + 1)
    cap = int(np.sort(box[box > 0])[(box > 0).sum() // 2])
    got, pth = _same(prots, sub, max_trace_cells=cap)
    assert ((pth["status"] == N.PATH_UNTRACED) == (box > cap)).all() and (pth["status"] == N.PATH_TRACED).sum() > 50
    assert (box == cap).any()                           # a box of exactly the cap is traced
    assert _same(prots, sub[:40], max_trace_cells=1)[1]["status"].max() <= N.PATH_UNTRACED


def test_a_3000_by_3000_pair_among_a_thousand_short_ones_and_alone(short_pairs):
    rng = np.random.default_rng(49)
    long_a = M.random_protein(rng, 3000)
    long_b = A.mutate(rng, long_a[:1400] + long_a[1420:] + M.random_protein(rng, 20), 0.2)
    assert len(long_b) == 3000 > LDS_COLS
    prots, pairs, aln, want = short_pairs
    n = len(prots)
    seq, off = M.pack(prots + [long_a, long_b])
    one = A.align_model(seq, off, [(n, n + 1)])
    wone = T.paths_model(seq, off, [(n, n + 1)], one)
    assert wone["status"][0] == N.PATH_TRACED and wone["gap_opens"][0] >= 1 and wone["identical"][0] > 2000
    words = -(-(int(one["end_a"][0]) + 1) // WAVE) * (-(-(int(one["end_b"][0]) + WAVE) // WORD)) * WAVE
    assert words * 4 > SHORT_SLAB and words * 4 * LONG_GRID > SLAB          # the second launch, narrowed by the slabs' total
    mixed = np.concatenate([pairs[:417], [(n, n + 1)], pairs[417:1000]])
    got, pth = _paths(prots + [long_a, long_b], mixed)
    assert got[417:418].tobytes() == one.tobytes() and pth[417:418].tobytes() == wone.tobytes()
    assert pth[:417].tobytes() == want[:417].tobytes() and pth[418:].tobytes() == want[417:1000].tobytes()
    got, pth = _paths(prots + [long_a, long_b], [(n, n + 1)])
    assert got.tobytes() == one.tobytes() and pth.tobytes() == wone.tobytes()
    # one cell under the box: untraced, beside the short ones
    box = (int(one["end_a"][0]) + 1) * (int(one["end_b"][0]) + 1)
    got, pth = _paths(prots + [long_a, long_b], mixed[400:430], max_trace_cells=box - 1)
    assert pth["status"][17] == N.PATH_UNTRACED and pth[:17].tobytes() == want[400:417].tobytes()


# ---- edge records -----------------------------------------------------------------------------------------------------------

def test_skipped_pairs_score_zero_and_nothing_to_trace():
    from kmergutsjava_amd import hotpath
    rng = np.random.default_rng(50)
    p64, p65 = M.random_protein(rng, 64), M.random_protein(rng, 65)
    got, pth = _same([p64, p65, b"XXXX", b"", b"ACDEFW"], [(0, 0), (0, 1), (1, 1), (2, 2), (3, 4), (4, 3), (4, 4), (2, 4)], max_cells=4096)
    assert got["status"].tolist() == [0, 1, 1, 0, 0, 0, 0, 0] and pth["status"].tolist() == [0, 1, 1, 1, 1, 1, 0, 1]
    assert pth[6].tolist() == (0, 0, 6, 6, 0, 0, 0, 0)
    aln, pth = hotpath.align_proteins(b"", np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32), paths=True)
    assert len(aln) == 0 and len(pth) == 0 and pth.dtype == N.ALIGN_PATH_DTYPE
    aln, pth = _paths([b"ACDEF"], np.zeros((0, 2), dtype=np.int32))
    assert len(aln) == 0 and len(pth) == 0
    # without the argument the return value is the records alone, and the same bytes
    seq, off = M.pack([p64, p65])
    assert hotpath.align_proteins(seq, off, [(0, 1), (1, 1)]).tobytes() == hotpath.align_proteins(seq, off, [(0, 1), (1, 1)], paths=True)[0].tobytes()


# ---- errors and allocations ---------------------------------------------------------------------------------------------------

def _raw(params, seq=b"ACDEFGHIKL", off=(0, 5, 10), pairs=(0, 1), n_pairs=None, out=True, paths=True, cap=1 << 24, device=False):
    lib = N.load()
    off = np.asarray(off, dtype=np.int64)
    pr = np.asarray(pairs, dtype=np.int32)
    n_pairs = len(pr) // 2 if n_pairs is None else n_pairs
    res = np.zeros(max(n_pairs, 1), dtype=N.ALIGNMENT_DTYPE)
    pth = np.zeros(max(n_pairs, 1), dtype=N.ALIGN_PATH_DTYPE)
    buf = np.frombuffer(seq, dtype=np.uint8)
    return lib.kg_proteins_align_paths(0, C.byref(params) if params is not None else None, buf.ctypes.data if seq else None, off.ctypes.data,
                                       len(off) - 1, pr.ctypes.data if len(pr) else None, n_pairs, cap, res.ctypes.data if out else None,
                                       pth.ctypes.data if paths else None)


def _error():
    return N.load().kg_last_error().decode()


def test_every_error_of_the_align_paths_call_with_its_first_words():
    ok = lambda **kw: N.KgAlignParams(**dict(dict(min_ratio_pct=50, ref=0, gap_open=11, gap_extend=1, max_cells=1 << 26, matrix=None, reserved=0), **kw))
    assert _raw(ok()) == 0
    for params, kw, code, words in [
            (None, {}, N.KG_ERR_ARG, "null kg_align_params"),
            (ok(min_ratio_pct=101), dict(cap=0), N.KG_ERR_ARG, "min_ratio_pct must be in 0..100"),       # the first bad one is named
            (ok(ref=2), {}, N.KG_ERR_ARG, "ref must be KG_ALIGN_REF_LONGER or KG_ALIGN_REF_MEMBER"),
            (ok(gap_open=-1), {}, N.KG_ERR_ARG, "gap_open must be >= 0"),
            (ok(gap_extend=0), {}, N.KG_ERR_ARG, "gap_extend must be >= 1"),
            (ok(max_cells=0), {}, N.KG_ERR_ARG, "max_cells must be >= 1"),
            (ok(reserved=1), {}, N.KG_ERR_ARG, "kg_align_params.reserved must be 0"),
            (ok(), dict(pairs=(0, 2)), N.KG_ERR_ARG, "pair 0: protein index 2 is outside [0, n_prot)"),
            (ok(), dict(off=(0, 6, 5)), N.KG_ERR_ARG, "protein 1: offsets decrease"),
            (ok(), dict(pairs=(), n_pairs=1), N.KG_ERR_ARG, "null argument"),
            (ok(), dict(out=False), N.KG_ERR_ARG, "null argument"),
            (ok(), dict(out=False, cap=0), N.KG_ERR_ARG, "null argument"),
            (ok(), dict(cap=0), N.KG_ERR_ARG, "max_trace_cells must be >= 1"),
            (ok(), dict(cap=-5, paths=False), N.KG_ERR_ARG, "max_trace_cells must be >= 1"),
            (ok(), dict(paths=False), N.KG_ERR_ARG, "null paths"),
            (ok(), dict(seq=b""), N.KG_ERR_ARG, "null sequence"),
            (ok(), dict(n_pairs=-1), N.KG_ERR_ARG, "n_pairs < 0"),
            (ok(), dict(off=(0, 1 << 24, (1 << 24) + 5)), N.KG_ERR_LIMIT, "protein 0: 2^24 or more characters")]:
        assert _raw(params, **kw) == code and _error().startswith(words), (words, _error())
    assert _raw(ok(), cap=1) == 0 and _raw(ok(), pairs=(), paths=False, out=False) == 0


def _relatives(rng, n_fam: int = 5):
    fam = [M.random_protein(rng, int(rng.integers(30, 90))) for _ in range(n_fam)]
    prots = []
    for _ in range(24):
        p = A.mutate(rng, fam[int(rng.integers(0, n_fam))], float(rng.choice([0.0, 0.05, 0.12, 0.25])))[int(rng.integers(0, 5)):]
        if rng.random() < 0.4:                          # a deletion or an insertion: gaps on the paths
            cut = int(rng.integers(5, len(p) - 5))
            p = p[:cut] + (b"" if rng.random() < 0.5 else M.random_protein(rng, 3)) + p[cut + int(rng.integers(0, 4)):]
        prots.append(p)
    prots += [M.random_protein(rng, int(rng.integers(0, 40))) for _ in range(6)] + [b"ACDEFGHIKX" * 3, b""]
    return [prots[i] for i in rng.permutation(len(prots))]


def _search(seq, off, n_db, **kw):
    from kmergutsjava_amd import hotpath
    return hotpath.search_proteins(seq, off, n_db, **kw)


def _raw_search(seq, off, n_db, trace=N.TRACE_HITS, cap=1 << 24, prm=(2, 8, 256, 0), al=(50, 0, 11, 1, 1 << 26, None, 0), max_pairs=0):
    lib = N.load()
    h = C.c_void_p()
    arr = np.frombuffer(bytes(seq), dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    p, a = N.KgSearchParams(*prm), N.KgAlignParams(*al)
    rc = lib.kg_proteins_search_paths(0, C.byref(p), C.byref(a), arr.ctypes.data, off.ctypes.data, len(off) - 1, n_db, 0, max_pairs, trace, cap,
                                      C.byref(h))
    msg = lib.kg_last_error().decode()
    if h.value:
        lib.kg_hitset_free(h)
    return rc, msg


def test_every_error_of_the_search_paths_call_and_of_the_getters():
    lib = N.load()
    seq, off = S.batch([b"ACDEFGHIKLMN", b"ACDEFGHIKLMN"])
    assert _raw_search(seq, off, 1)[0] == 0
    for kw, words in [(dict(trace=0), "trace must be KG_TRACE_HITS or KG_TRACE_ALL"), (dict(trace=3), "trace must be KG_TRACE_HITS or KG_TRACE_ALL"),
                      (dict(trace=3, cap=0), "trace must be KG_TRACE_HITS or KG_TRACE_ALL"), (dict(cap=0), "max_trace_cells must be >= 1"),
                      (dict(max_pairs=-1, cap=0), "max_pairs must be >= 0"), (dict(prm=(0, 8, 256, 0), trace=9), "min_shared must be >= 1"),
                      (dict(al=(50, 0, 11, 1, 0, None, 0), cap=0), "max_cells must be >= 1"), (dict(n_db=3), "n_db must be in 0..n_prot")]:
        kw = dict(kw)
        rc, msg = _raw_search(seq, off, kw.pop("n_db", 1), **kw)
        assert rc == N.KG_ERR_ARG and msg.startswith(words), (kw, rc, msg)
    # a set made by the old call has no paths
    h = C.c_void_p()
    arr = np.frombuffer(seq, dtype=np.uint8)
    p, a = N.KgSearchParams(2, 8, 256, 0), N.KgAlignParams(50, 0, 11, 1, 1 << 26, None, 0)
    assert lib.kg_proteins_search(0, C.byref(p), C.byref(a), arr.ctypes.data, off.ctypes.data, 2, 1, 0, 0, C.byref(h)) == 0
    try:
        assert lib.kg_hitset_count(h) == 1
        dst, st = np.zeros(1, dtype=N.ALIGN_PATH_DTYPE), N.KgTraceStats()
        assert lib.kg_hitset_paths_copy(h, 0, 1, dst.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_hitset_paths_copy: the set was made without paths")
        assert lib.kg_hitset_trace_stats(h, C.byref(st)) == N.KG_ERR_ARG and _error().startswith("kg_hitset_trace_stats: the set was made without paths")
    finally:
        lib.kg_hitset_free(h)
    assert lib.kg_proteins_search_paths(0, C.byref(p), C.byref(a), arr.ctypes.data, off.ctypes.data, 2, 1, 0, 0, N.TRACE_ALL, 1 << 24, C.byref(h)) == 0
    try:
        dst = np.zeros(1, dtype=N.ALIGN_PATH_DTYPE)
        assert lib.kg_hitset_paths_copy(h, 0, 1, dst.ctypes.data) == 0 and dst[0].tolist() == (0, 0, 12, 12, 0, 0, 0, 0)
        assert lib.kg_hitset_paths_copy(h, 1, 1, dst.ctypes.data) == N.KG_ERR_ARG and _error().startswith("kg_hitset_paths_copy: range outside the set")
        assert lib.kg_hitset_paths_copy(h, 0, 1, None) == N.KG_ERR_ARG and _error().startswith("null argument")
    finally:
        lib.kg_hitset_free(h)
    assert lib.kg_hitset_paths_copy(None, 0, 0, None) == N.KG_ERR_ARG and lib.kg_hitset_trace_stats(None, None) == N.KG_ERR_ARG


def test_failed_allocations_leave_nothing_behind(monkeypatch, short_pairs):
    import torch
    from kmergutsjava_amd import hotpath, synth
    prots, pairs, aln, want = short_pairs
    prots = prots + [M.random_protein(np.random.default_rng(51), LDS_COLS + 1)]         # the carry of the second launch too
    pairs = np.concatenate([pairs[:50], [(len(prots) - 1, len(prots) - 1)]])
    seq, off = M.pack(prots)
    mat = np.array(AS.BLOSUM62)
    rec = synth.high_density_config(4, 100, 4001, 500, dna=False)[2]
    sseq, soff = S.batch(_relatives(np.random.default_rng(52)))
    with hotpath.SignatureTable.from_bytes(synth.table_image(rec), 0) as tab:
        first = hotpath.align_proteins(seq, off, pairs, matrix=mat, paths=True)
        assert first[1][:50].tobytes() == want[:50].tobytes() and first[1][50].tolist() == (0, 0, LDS_COLS + 1, LDS_COLS + 1, 0, 0, 0, 0)
        sfirst = _search(sseq, soff, 16, paths="all")
        plain = 0
        for n in range(1, 600):                         # how many allocations the search without paths makes
            monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
            try:
                _search(sseq, soff, 16)
                break
            except N.KmerGutsNativeError:
                plain += 1
        monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
        torch.cuda.synchronize()
        free0, live0 = torch.cuda.mem_get_info()[0], tab.live_device_bytes()
        for call, want_failed in ((lambda: hotpath.align_proteins(seq, off, pairs, matrix=mat, paths=True), 8 + 6),
                                  (lambda: _search(sseq, soff, 16, paths="all"), plain + 5)):
            failed = 0
            for n in range(1, 700):
                monkeypatch.setenv("KG_TEST_FAIL_ALLOC", str(n))
                try:
                    got = call()
                    break
                except N.KmerGutsNativeError as e:
                    assert e.code == N.KG_ERR_NOMEM, e
                    failed += 1
                    assert torch.cuda.mem_get_info()[0] == free0, "allocation %d failed and device memory stayed in use" % n
                    assert tab.live_device_bytes() == live0
            monkeypatch.delenv("KG_TEST_FAIL_ALLOC")
            # align_run's eight, then the jobs, the words, the records, the direction words, the matrix and the carry; the search:
            # the path block, the jobs, the words, the records and the direction words
            assert failed == want_failed, (failed, want_failed)
            assert torch.cuda.mem_get_info()[0] == free0 and tab.live_device_bytes() == live0
        assert got[0].tobytes() == sfirst[0].tobytes() and got[2].tobytes() == sfirst[2].tobytes()


# ---- search -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_random_batches_with_planted_relatives_under_both_trace_modes(seed):
    rng = np.random.default_rng(200 + seed)
    prots = _relatives(rng)
    n_db = int(rng.integers(0, len(prots) + 1)) if seed % 6 else len(prots) // 2
    align = dict(min_ratio_pct=int(rng.choice([0, 30, 50, 100])), ref=str(rng.choice(["longer", "member"])),
                 max_cells=int(rng.choice([2000, 1 << 26])), gap_open=int(rng.choice([11, 0, 5])))
    kw = dict(min_shared=int(rng.integers(1, 4)), max_cand=int(rng.choice([1, 2, 3, 8, 64])), max_db_per_kmer=int(rng.choice([1, 2, 4, 256])))
    cap = int(rng.choice([1 << 24, 1500]))
    seq, off = S.batch(prots)
    searched = S.search_model(seq, off, n_db, **kw, **align)
    old = _search(seq, off, n_db, align=align, **kw)
    assert old[0].tobytes() == searched[0].tobytes()
    for mode in ("hits", "all"):
        whits, wstart, wpth, wst = T.search_paths_model(seq, off, n_db, mode, cap, searched=searched, **kw, **align)
        hits, start, pth, st = _search(seq, off, n_db, align=align, paths=mode, max_trace_cells=cap, **kw)
        assert hits.tobytes() == whits.tobytes() == old[0].tobytes() and start.tobytes() == wstart.tobytes() == old[1].tobytes()
        bad = np.flatnonzero(pth != wpth)
        assert pth.tobytes() == wpth.tobytes(), (mode, bad[:5], pth[bad[:5]], wpth[bad[:5]], hits[bad[:5]])
        assert {k: st[k] for k in S.STAT_KEYS} == {k: wst[k] for k in S.STAT_KEYS} == {k: old[2][k] for k in S.STAT_KEYS}
        assert (st["traced"], st["untraced"], st["trace_cells"]) == (wst["traced"], wst["untraced"], wst["trace_cells"])
        if mode == "hits":
            assert (pth["status"][hits["status"] != N.SEARCH_HIT] == N.PATH_NONE).all()


def test_the_device_sequence_entry_points():
    import torch
    from kmergutsjava_amd import hotpath
    seq, off = S.batch(_relatives(np.random.default_rng(53)))
    want = _search(seq, off, 12, paths="all")
    dev = torch.from_numpy(np.frombuffer(seq, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = _search(None, off, 12, device_ptr=dev.data_ptr(), paths="all")
    assert all(got[k].tobytes() == want[k].tobytes() for k in range(3)) and got[3]["traced"] == want[3]["traced"] > 5
    pairs = [(a, b) for a in range(12, 20) for b in range(0, 12, 3)]
    a1, p1 = hotpath.align_proteins(seq, off, pairs, paths=True)
    a2, p2 = hotpath.align_proteins(None, off, pairs, paths=True, device_ptr=dev.data_ptr())
    assert a1.tobytes() == a2.tobytes() and p1.tobytes() == p2.tobytes()


def test_end_to_end_with_paths(tmp_path):
    """The golden E. coli proteome as the database; 192 of its proteins as queries with a substitution at every 12th residue, and
    in every fourth of them three residues of the middle deleted; search_proteins --paths as a subprocess.  What a rank-0 hit on
    the query's own original must show is computed here from the planted edits with the model."""
    from kmergutsjava_amd.make_signatures import _read, parse_fasta
    faa = os.path.join(ROOT, "tests", "golden", "Ecoli_K12_W3110.faa.gz")
    ids, seqs = parse_fasta(_read(faa), faa)
    assert max(len(s) for s in seqs) < 4096                  # every box is below 2^24 cells: no hit can be untraced
    pick = [k for k in range(0, len(ids), len(ids) // 260) if 60 <= len(seqs[k]) <= 700][:192]
    assert len(pick) == 192
    alpha = A.ALPHA
    queries, planted = [], {}
    for n, k in enumerate(pick):
        p = seqs[k]
        q = bytes(alpha[(alpha.index(ch) + 3) % 20] if i % 12 == 6 and ch in alpha else ch for i, ch in enumerate(p))
        deleted = n % 4 == 0
        if deleted:
            q = q[:len(q) // 2] + q[len(q) // 2 + 3:]
        queries.append(q)
        planted[b"m_" + ids[k]] = (p, q, deleted)
    (tmp_path / "q.faa").write_bytes(b"".join(b">m_%s\n%s\n" % (ids[k], q) for k, q in zip(pick, queries)))
    out = tmp_path / "hits.tsv"
    r = subprocess.run([sys.executable, "-m", "kmergutsjava_amd.search_proteins", "-d", faa, "-q", str(tmp_path / "q.faa"), "-o", str(out),
                        "--paths"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = r.stderr.strip().splitlines()[-1]
    m = re.search(r"hits: (\d+), queries hit: (\d+), .*, traced: (\d+), untraced: (\d+), trace ms: ([0-9.]+)$", line)
    assert m, line
    hits, q_hit, traced, untraced = map(int, m.groups()[:4])
    assert untraced == 0 and traced == hits >= q_hit >= 0.9 * len(pick)
    rows = [x.split(b"\t") for x in out.read_bytes().splitlines()]
    assert len(rows) == q_hit and all(len(x) == 20 and x[1] == b"0" and x[9] == b"hit" and b"-" not in x[10:] for x in rows)
    seq_of = dict(zip(ids, seqs))
    own = 0
    for x in rows:
        p, q, deleted = planted[x[0]]
        if seq_of[x[2]] != p:
            continue
        own += 1
        got = [int(v) for v in x[10:20]]
        end, rec = T.trace_numpy(q, p)
        assert (end[1] + 1, end[2] + 1) == (int(x[7]), int(x[8])) and end[0] == int(x[4])
        ra, rb, columns = T.columns_of(end, rec)
        assert got == [rec[0] + 1, rec[1] + 1, columns, rec[2], 100 * rec[2] // columns, rec[3], rec[4], rec[5] + rec[6],
                       100 * (end[1] - rec[0] + 1) // len(q), 100 * (end[2] - rec[1] + 1) // len(p)], (x, rec)
        # from the planted edits: a gap exactly where a deletion was planted (the original's three residues face nothing:
        # columns (-, b_j)), and every residue that was neither substituted nor deleted identical
        kept = [i for i in range(len(p)) if not (deleted and len(p) // 2 <= i < len(p) // 2 + 3)]
        same = sum(1 for i in kept if not (i % 12 == 6 and p[i] in alpha))
        # (the path has at most len(p) columns: the query's residues and the three the deletion took)
        assert (got[6] >= 1) == deleted and got[3] >= same and (got[7] == 3) == deleted, (x, deleted, same)
        assert got[2] <= len(p) and got[4] >= 100 * same // len(p)
    assert own >= 0.9 * len(pick)
